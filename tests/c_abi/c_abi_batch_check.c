/*
 * tests/c_abi/c_abi_batch_check.c -- training batches from decoded images (gsasr_batch_make, gsasr_batch_pick) from plain C: no
 * Python, no torch.
 *
 * Three 13 x 13 windows of one 17 x 19 BGR image, on an address one byte past a dword, go to GT slots of 15 x 16 and LR images of
 * 6 x 6 through the header alone: un-augmented, flipped both ways, and flipped horizontally + transposed.  GT must equal
 * (float)byte / 255.0f through the header's index map exactly, zeros in the padding included; LR is held to the header's resize
 * formulas evaluated here in double on the un-augmented window, then augmented, bar 2e-6 (two passes * (11 taps + the weight's
 * and the store's rounding) * 2^-24 * sum|w| 1.25 = 2e-6); the picked pixels must equal the GT's, a wrapped and an out-of-range
 * point included.  Then each documented argument error.  Built and run by tests/test_make_batch_gpu.py on the GPU box.
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

enum { B = 3, SH = 17, SW = 19, N = 13, M = 6, GH = 15, GW = 16, P = 11, S = 5 };

static unsigned lcg_state = 77u;
static unsigned char lcg_byte(void) { lcg_state = lcg_state * 1664525u + 1013904223u; return (unsigned char)(lcg_state >> 24); }

static double cubic(double x)
{
    const double a = fabs(x);
    if (a <= 1.0) return 1.5 * a * a * a - 2.5 * a * a + 1.0;
    if (a <= 2.0) return -0.5 * a * a * a + 2.5 * a * a - 4.0 * a + 2.0;
    return 0.0;
}

static double A[M][N];      /* the axis' map, dense: both axes are 13 -> 6 */

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

static const int win[4 * B] = {2, 3, N, N, 4, 6, N, N, 0, 0, N, N};
static const unsigned char aug[B] = {0, GSASR_BATCH_HFLIP | GSASR_BATCH_VFLIP, GSASR_BATCH_HFLIP | GSASR_BATCH_TRANSPOSE};

/* pixel (r, c) of augmented sample b -> (row, column) of its window */
static void source_of(int b, int r, int c, int *cy, int *cx)
{
    const int fr = (aug[b] & GSASR_BATCH_TRANSPOSE) ? c : r, fc = (aug[b] & GSASR_BATCH_TRANSPOSE) ? r : c;
    *cy = (aug[b] & GSASR_BATCH_VFLIP) ? N - 1 - fr : fr;
    *cx = (aug[b] & GSASR_BATCH_HFLIP) ? N - 1 - fc : fc;
}

int main(void)
{
    if (build_matrix()) { printf("host weights failed\n"); return 1; }
    static unsigned char img[SH * SW * 3];
    for (int i = 0; i < SH * SW * 3; ++i) img[i] = lcg_byte();
    unsigned char *d_buf;
    float *d_gt, *d_lq, *d_pick;
    int *d_pts;
    CK(hipMalloc((void **)&d_buf, sizeof img + 8));
    unsigned char *d_img = d_buf + 1;
    CK(hipMemcpy(d_img, img, sizeof img, hipMemcpyHostToDevice));
    const size_t n_gt = (size_t)B * 3 * GH * GW, n_lq = (size_t)B * 3 * M * M;
    CK(hipMalloc((void **)&d_gt, n_gt * sizeof(float))); CK(hipMalloc((void **)&d_lq, n_lq * sizeof(float)));
    CK(hipMalloc((void **)&d_pick, (size_t)B * 3 * S * sizeof(float))); CK(hipMalloc((void **)&d_pts, (size_t)B * S * 2 * sizeof(int)));
    CK(hipMemset(d_gt, 0xff, n_gt * sizeof(float)));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    int bad = 0;
    const unsigned char *srcs[B] = {d_img, d_img, d_img};
    const int src_hw[2 * B] = {SH, SW, SH, SW, SH, SW};
    gsasr_batch d;
    memset(&d, 0, sizeof d);
    d.batch = B; d.src = srcs; d.src_hw = src_hw; d.window = win; d.aug = aug;
    d.gt_h = GH; d.gt_w = GW; d.gt = d_gt; d.lr_h = M; d.lr_w = M; d.lq = d_lq; d.flags = GSASR_BATCH_BGR;
    const size_t bytes = gsasr_batch_scratch_bytes(&d);
    if (bytes < (size_t)B * 3 * N * N * sizeof(float) || bytes % 256) { printf("scratch bytes %zu\n", bytes); bad = 1; }
    void *scratch;
    CK(hipMalloc(&scratch, bytes ? bytes : 256));
    d.scratch = scratch;
    OK(gsasr_batch_make(&d, st));
    CK(hipStreamSynchronize(st));
    static float gt[B * 3 * GH * GW], lq[B * 3 * M * M];
    CK(hipMemcpy(gt, d_gt, sizeof gt, hipMemcpyDeviceToHost));
    CK(hipMemcpy(lq, d_lq, sizeof lq, hipMemcpyDeviceToHost));
    int wrong = 0;
    double worst = 0.0;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < 3; ++p) {
            /* the un-augmented window's plane p (r, g, b from bytes b, g, r), rows then columns in double */
            static double x[N][N], tmp[M][N], y[M][M];
            for (int r = 0; r < N; ++r)
                for (int c = 0; c < N; ++c)
                    x[r][c] = (double)((float)img[((win[4 * b] + r) * SW + win[4 * b + 1] + c) * 3 + 2 - p] / 255.0f);
            for (int o = 0; o < M; ++o)
                for (int c = 0; c < N; ++c) { double a = 0.0; for (int k = 0; k < N; ++k) a += A[o][k] * x[k][c]; tmp[o][c] = a; }
            for (int o = 0; o < M; ++o)
                for (int q = 0; q < M; ++q) { double a = 0.0; for (int k = 0; k < N; ++k) a += A[q][k] * tmp[o][k]; y[o][q] = a; }
            for (int r = 0; r < GH; ++r)
                for (int c = 0; c < GW; ++c) {
                    float want = 0.0f;
                    if (r < N && c < N) { int cy, cx; source_of(b, r, c, &cy, &cx); want = (float)x[cy][cx]; }
                    if (memcmp(&gt[((b * 3 + p) * GH + r) * GW + c], &want, sizeof want)) ++wrong;
                }
            for (int r = 0; r < M; ++r)
                for (int c = 0; c < M; ++c) {
                    const int fr = (aug[b] & GSASR_BATCH_TRANSPOSE) ? c : r, fc = (aug[b] & GSASR_BATCH_TRANSPOSE) ? r : c;
                    const int cy = (aug[b] & GSASR_BATCH_VFLIP) ? M - 1 - fr : fr, cx = (aug[b] & GSASR_BATCH_HFLIP) ? M - 1 - fc : fc;
                    const double e = fabs((double)lq[((b * 3 + p) * M + r) * M + c] - y[cy][cx]);
                    if (!(e <= worst)) worst = e;
                }
        }
    printf("3 windows of 13 x 13 in slots of %d x %d: %d GT values differ; LR 6 x 6: max error against double %.3e (bar 2e-6)\n", GH, GW, wrong, worst);
    if (wrong || !(worst <= 2e-6)) bad = 1;
    /* the picked pixels: two inside, the last row and first column by wrapping, one out of range, one out of range after the wrap */
    static const int one[2 * S] = {0, 0, 7, 12, -1, -N, N, 0, 3, -N - 1};
    int pts[B * S * 2];
    for (int b = 0; b < B; ++b) memcpy(pts + b * S * 2, one, sizeof one);
    CK(hipMemcpy(d_pts, pts, sizeof pts, hipMemcpyHostToDevice));
    OK(gsasr_batch_pick(&d, d_pts, S, d_pick, st));
    CK(hipStreamSynchronize(st));
    float pick[B * 3 * S];
    CK(hipMemcpy(pick, d_pick, sizeof pick, hipMemcpyDeviceToHost));
    static const int at[2 * S] = {0, 0, 7, 12, N - 1, 0, -1, -1, -1, -1};
    wrong = 0;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < 3; ++p)
            for (int i = 0; i < S; ++i) {
                const float want = at[2 * i] < 0 ? 0.0f : gt[((b * 3 + p) * GH + at[2 * i]) * GW + at[2 * i + 1]];
                if (memcmp(&pick[(b * 3 + p) * S + i], &want, sizeof want)) ++wrong;
            }
    printf("%d picked values differ from the GT's\n", wrong);
    if (wrong) bad = 1;
    /* argument errors: status + message, nothing enqueued */
#define REFUSED(what, stmt)                                                                                       \
    do {                                                                                                          \
        gsasr_batch e = d; int w2[4 * B]; int hw2[2 * B]; unsigned char a2[B]; const unsigned char *s2[B];       \
        memcpy(w2, win, sizeof w2); memcpy(hw2, src_hw, sizeof hw2); memcpy(a2, aug, sizeof a2); memcpy(s2, srcs, sizeof s2); \
        e.window = w2; e.src_hw = hw2; e.aug = a2; e.src = s2;                                                     \
        stmt;                                                                                                     \
        if (gsasr_batch_make(&e, st) != GSASR_ERR_ARG || !gsasr_last_error()[0]) { printf("%s accepted\n", what); bad = 1; } \
    } while (0)
    REFUSED("batch 0", e.batch = 0);
    REFUSED("batch 65", e.batch = GSASR_MAX_BATCH + 1);
    REFUSED("null src array", e.src = NULL);
    REFUSED("null source image", s2[1] = NULL);
    REFUSED("null src_hw", e.src_hw = NULL);
    REFUSED("null window", e.window = NULL);
    REFUSED("null lq", e.lq = NULL);
    REFUSED("null scratch", e.scratch = NULL);
    REFUSED("misaligned gt", e.gt = (float *)((char *)d_gt + 2));
    REFUSED("misaligned lq", e.lq = (float *)((char *)d_lq + 1));
    REFUSED("misaligned scratch", e.scratch = (char *)scratch + 16);
    REFUSED("window below its source", w2[0] = SH - N + 1);
    REFUSED("window right of its source", w2[5] = SW - N + 1);
    REFUSED("negative window offset", w2[8] = -1);
    REFUSED("window with no pixel", w2[2] = 0);
    REFUSED("source of 0 rows", hw2[0] = 0);
    REFUSED("source of 32768 columns", hw2[1] = 32768);
    REFUSED("gt_h 32768", e.gt_h = 32768);
    REFUSED("lr_w 0", e.lr_w = 0);
    REFUSED("GT slot smaller than a sample", e.gt_w = N - 1);
    REFUSED("transposed sample with a rectangular LR", e.lr_w = M + 1);
    REFUSED("unknown flag", e.flags |= 4u);
    REFUSED("unknown augmentation bit", a2[0] = 8);
    REFUSED("reflection condition", (e.lr_h = 1, a2[2] = 0));
    if (!strstr(gsasr_last_error(), "reflection")) { printf("the reflection condition's message is missing\n"); bad = 1; }
    { gsasr_batch e = d; e.lr_h = 1; if (gsasr_batch_scratch_bytes(&e) != 0) { printf("scratch bytes of a refused descriptor\n"); bad = 1; } }
    if (gsasr_batch_make(NULL, st) != GSASR_ERR_ARG || gsasr_batch_scratch_bytes(NULL) != 0 || gsasr_batch_pick(NULL, d_pts, S, d_pick, st) != GSASR_ERR_ARG) {
        printf("null descriptor accepted\n"); bad = 1;
    }
    if (gsasr_batch_pick(&d, NULL, S, d_pick, st) != GSASR_ERR_ARG || gsasr_batch_pick(&d, d_pts, S, NULL, st) != GSASR_ERR_ARG ||
        gsasr_batch_pick(&d, d_pts, 0, d_pick, st) != GSASR_ERR_ARG || gsasr_batch_pick(&d, (int *)((char *)d_pts + 2), S, d_pick, st) != GSASR_ERR_ARG) {
        printf("bad pick arguments accepted\n"); bad = 1;
    }
    /* a null gt is allowed: only lq is made */
    { gsasr_batch e = d; e.gt = NULL; OK(gsasr_batch_make(&e, st)); CK(hipStreamSynchronize(st)); }
    static float lq2[B * 3 * M * M];
    CK(hipMemcpy(lq2, d_lq, sizeof lq2, hipMemcpyDeviceToHost));
    if (memcmp(lq, lq2, sizeof lq)) { printf("a second call gave other bits\n"); bad = 1; }
    if (gsasr_abi_version() != 7) { printf("ABI version changed\n"); bad = 1; }
    printf("%s\n", bad ? "C-ABI BATCH CHECK FAILED" : "C-ABI BATCH CHECK OK");
    return bad;
}
