/*
 * tests/c_abi/c_abi_resize_check.c -- the bicubic imresize (gsasr_imresize) from plain C: no Python, no torch.
 *
 * Two samples of 3 x 53 x 53 in [0,1], in a buffer whose rows are 61 floats apart, to 48 x 48 at scale 48/53 through the header
 * alone, against the formulas of include/gsasr_splat.h evaluated here in double (weights, single reflection, rows then
 * columns).  Bar 2e-6: two passes * (7 taps + the weight's and the store's rounding) * 2^-24 * sum|w| 1.25 = 1.4e-6.  Then
 * the adjoint's inner product, <A x, y> = <x, A^T y> to 1e-5 relative, and the descriptor's argument errors.  Built and run by
 * tests/test_imresize_gpu.py on the GPU box.
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

enum { B = 2, C = 3, N = 53, M = 48, PITCH = 61, P = 7 };

static unsigned lcg_state = 2024u;
static float lcg01(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) / 16777216.0f; }

static double cubic(double x)
{
    const double a = fabs(x);
    if (a <= 1.0) return 1.5 * a * a * a - 2.5 * a * a + 1.0;
    if (a <= 2.0) return -0.5 * a * a * a + 2.5 * a * a - 4.0 * a + 2.0;
    return 0.0;
}

static double A[M][N];      /* the axis' map, dense: both axes are 53 -> 48 */

static int build_matrix(void)
{
    const double s = (double)M / N, kw = 4.0 / s;
    if ((int)ceil(kw) + 2 != P) return 1;
    memset(A, 0, sizeof A);
    for (int o = 1; o <= M; ++o) {
        const double u = o / s + 0.5 * (1.0 - 1.0 / s), left = floor(u - kw / 2.0);
        double w[P], sum = 0.0;
        for (int t = 0; t < P; ++t) { w[t] = s * cubic((u - (left + t)) * s); sum += w[t]; }
        for (int t = 0; t < P; ++t) {
            int k = (int)left + t - 1;
            k = k < 0 ? -1 - k : k >= N ? 2 * N - 1 - k : k;
            if (k < 0 || k >= N) { if (w[t] != 0.0) return 1; continue; }
            A[o - 1][k] += w[t] / sum;
        }
    }
    return 0;
}

int main(void)
{
    if (build_matrix()) { printf("host weights failed\n"); return 1; }
    const size_t n_in = (size_t)B * C * N * PITCH, n_out = (size_t)B * C * M * M;
    float *x = malloc(n_in * sizeof(float)), *y = malloc(n_out * sizeof(float)), *g = malloc(n_out * sizeof(float)), *gx = malloc(n_in * sizeof(float));
    for (size_t i = 0; i < n_in; ++i) x[i] = lcg01();
    for (size_t i = 0; i < n_out; ++i) g[i] = 2.0f * lcg01() - 1.0f;
    float *d_x, *d_y, *d_g, *d_gx;
    CK(hipMalloc((void **)&d_x, n_in * sizeof(float))); CK(hipMalloc((void **)&d_y, n_out * sizeof(float)));
    CK(hipMalloc((void **)&d_g, n_out * sizeof(float))); CK(hipMalloc((void **)&d_gx, n_in * sizeof(float)));
    CK(hipMemcpy(d_x, x, n_in * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_g, g, n_out * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemset(d_gx, 0, n_in * sizeof(float)));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    int bad = 0;
    const double scales[2] = {(double)M / N, (double)M / N};
    gsasr_resize r;
    memset(&r, 0, sizeof r);
    r.batch = B; r.channels = C; r.in_h = N; r.in_w = N; r.out_h = M; r.out_w = M;
    r.scales = scales; r.flags = GSASR_RESIZE_SHARED_SCALE;
    r.in = d_x; r.in_pitch = PITCH * sizeof(float); r.in_plane = (size_t)N * PITCH * sizeof(float); r.in_stride = C * r.in_plane;
    r.out = d_y; r.out_pitch = M * sizeof(float); r.out_plane = (size_t)M * M * sizeof(float); r.out_stride = C * r.out_plane;
    const size_t bytes = gsasr_resize_scratch_bytes(&r);
    if (bytes < (size_t)B * C * M * N * sizeof(float)) { printf("scratch bytes %zu\n", bytes); bad = 1; }
    void *scratch;
    CK(hipMalloc(&scratch, bytes ? bytes : 16));
    r.scratch = scratch;
    OK(gsasr_imresize(&r, st));
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(y, d_y, n_out * sizeof(float), hipMemcpyDeviceToHost));
    /* rows first, then columns, in double */
    static double tmp[M][N];
    double worst = 0.0, dot_y = 0.0, dot_scale = 0.0;
    for (int z = 0; z < B * C; ++z) {
        const float *src = x + (size_t)z * N * PITCH;
        for (int o = 0; o < M; ++o)
            for (int c = 0; c < N; ++c) {
                double a = 0.0;
                for (int k = 0; k < N; ++k) a += A[o][k] * (double)src[(size_t)k * PITCH + c];
                tmp[o][c] = a;
            }
        for (int o = 0; o < M; ++o)
            for (int q = 0; q < M; ++q) {
                double a = 0.0;
                for (int k = 0; k < N; ++k) a += A[q][k] * tmp[o][k];
                const size_t i = ((size_t)z * M + o) * M + q;
                const double e = fabs((double)y[i] - a);
                if (e > worst) worst = e;
                dot_y += (double)y[i] * (double)g[i];
                dot_scale += fabs((double)y[i] * (double)g[i]);
            }
    }
    printf("53 -> 48, 2 x 3 planes, pitch %d floats: max error against double %.3e (bar 2e-6)\n", PITCH, worst);
    if (!(worst <= 2e-6)) bad = 1;
    /* the adjoint: grad_out = g, grad_in into the pitched buffer */
    r.in = d_gx; r.out = d_g;
    OK(gsasr_imresize_backward(&r, st));
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(gx, d_gx, n_in * sizeof(float), hipMemcpyDeviceToHost));
    double dot_x = 0.0;
    int touched = 0;
    for (int z = 0; z < B * C; ++z)
        for (int k = 0; k < N; ++k)
            for (int c = 0; c < PITCH; ++c) {
                const size_t i = ((size_t)z * N + k) * PITCH + c;
                if (c < N) dot_x += (double)x[i] * (double)gx[i];
                else if (gx[i] != 0.0f) touched = 1;
            }
    printf("<A x, y> = %.9e, <x, A^T y> = %.9e (difference %.3e of %.3e)\n", dot_y, dot_x, fabs(dot_y - dot_x), dot_scale);
    if (!(fabs(dot_y - dot_x) <= 1e-5 * dot_scale) || touched) { if (touched) printf("the backward wrote between the rows\n"); bad = 1; }
    /* argument errors: status + message, nothing enqueued */
    r.in = d_x; r.out = d_y;
    gsasr_resize e = r;
    e.in_pitch = N * sizeof(float) - 4;
    if (gsasr_imresize(&e, st) != GSASR_ERR_ARG || gsasr_resize_scratch_bytes(&e) != 0) { printf("short pitch accepted\n"); bad = 1; }
    e = r; e.flags |= 8u;
    if (gsasr_imresize(&e, st) != GSASR_ERR_ARG) { printf("unknown flag accepted\n"); bad = 1; }
    e = r; e.in_h = 26; e.in_w = 26; e.out_h = 2; e.out_w = 2;
    const double sixteenth[2] = {1.0 / 16, 1.0 / 16};
    e.scales = sixteenth;
    if (gsasr_imresize(&e, st) != GSASR_ERR_ARG || !strstr(gsasr_last_error(), "reflection")) { printf("26 pixels at 1/16 accepted\n"); bad = 1; }
    e = r; e.out = NULL;
    if (gsasr_imresize(&e, st) != GSASR_ERR_ARG) { printf("null out accepted\n"); bad = 1; }
    e = r; e.flags |= GSASR_RESIZE_ACCUMULATE;
    if (gsasr_imresize(&e, st) != GSASR_ERR_ARG) { printf("ACCUMULATE accepted by the forward\n"); bad = 1; }
    if (gsasr_imresize(NULL, st) != GSASR_ERR_ARG || gsasr_resize_scratch_bytes(NULL) != 0) { printf("null descriptor accepted\n"); bad = 1; }
    if (gsasr_abi_version() != 7) { printf("ABI version changed\n"); bad = 1; }
    printf("%s\n", bad ? "C-ABI RESIZE CHECK FAILED" : "C-ABI RESIZE CHECK OK");
    return bad;
}
