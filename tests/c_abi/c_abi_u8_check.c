/*
 * tests/c_abi/c_abi_u8_check.c -- the 8-bit forward (gsasr_splat_forward_u8) from plain C: no Python, no torch.
 *
 * Gaussians on a 64-px lattice whose windows (explicit cutoff 6: 3.5 sigma of <= 4 px) do not overlap, so every pixel
 * is one term and the float image of gsasr_splat_forward on the same plan is reproducible: the bytes must equal
 * rintf(fminf(fmaxf(v, 0), 1) * 255) of it exactly -- inside a crop that is no multiple of 8 or 16, with swapped channels, a
 * pitch wider than the row and a canary pattern around the pixels that must survive.  Then the argument errors.  Built and
 * run by tests/test_u8_output_gpu.py on the GPU box.
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

int main(void)
{
    enum { H = 192, W = 256, NY = 3, NX = 4, S = NY * NX, ROWS = 171, COLS = 219, PAD = 13, EXTRA = 2 };
    const size_t pitch = 3 * COLS + PAD, nbuf = (size_t)(ROWS + EXTRA) * pitch;
    const float colours[4][3] = {{1.3f, -0.4f, 0.9f}, {0.35f, 1.0f, 2.5f}, {-1.0f, 0.6f, 1.1f}, {5.0f, 0.08f, 0.999f}};
    float sig[3 * S], xy[2 * S], col[3 * S];
    for (int i = 0; i < S; ++i) {
        const double px = (i % NX + 0.5) * 64 + 0.37 * (i % 3), py = (i / NX + 0.5) * 64 - 0.21 * (i % 4);
        sig[3 * i + 0] = (float)((3.2 + 0.2 * (i % 4)) * 2 / (W - 1));
        sig[3 * i + 1] = (float)((4.0 - 0.2 * (i % 3)) * 2 / (H - 1));
        sig[3 * i + 2] = 0.1f * (float)(i % 7) - 0.3f;
        xy[2 * i + 0] = (float)(px * 2 / (W - 1) - 1);
        xy[2 * i + 1] = (float)(py * 2 / (H - 1) - 1);
        for (int k = 0; k < 3; ++k) col[3 * i + k] = colours[i % 4][k];
    }
    float *d_sig, *d_xy, *d_col, *d_img;
    unsigned char *d_out;
    CK(hipMalloc((void **)&d_sig, sizeof sig)); CK(hipMalloc((void **)&d_xy, sizeof xy)); CK(hipMalloc((void **)&d_col, sizeof col));
    CK(hipMalloc((void **)&d_img, sizeof(float) * 3 * H * W)); CK(hipMalloc((void **)&d_out, nbuf));
    CK(hipMemcpy(d_sig, sig, sizeof sig, hipMemcpyHostToDevice)); CK(hipMemcpy(d_xy, xy, sizeof xy, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_col, col, sizeof col, hipMemcpyHostToDevice));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    float *img = malloc(sizeof(float) * 3 * H * W);
    unsigned char *canary = malloc(nbuf), *out = malloc(nbuf);
    for (size_t i = 0; i < nbuf; ++i) canary[i] = (unsigned char)(i % 251);
    int bad = 0;
    const float dmaxs[2] = {40.0f / (W - 1), -1.f};     /* a box of <= 20 px each way; the unbounded op */
    for (int v = 0; v < 2; ++v) {
        /* GSASR_FLAG_CHW_IMAGE on the dims: ignored by the u8 call, honoured by nobody here (the float call gets its own dims) */
        gsasr_dims d = {S, H, W, 3, dmaxs[v], 0, H, 6.0f, GSASR_FLAG_FORWARD_ONLY | GSASR_FLAG_CHW_IMAGE};
        gsasr_dims df = d;
        df.flags = GSASR_FLAG_FORWARD_ONLY | GSASR_FLAG_OVERWRITE_IMAGE;
        const size_t bytes = gsasr_splat_workspace_bytes(&d);
        void *ws;
        CK(hipMalloc(&ws, bytes));
        OK(gsasr_splat_plan(d_sig, d_xy, d_col, &d, ws, bytes, st));
        OK(gsasr_splat_forward(&df, ws, bytes, d_img, st));
        for (unsigned flags = 0; flags < 2; ++flags) {
            CK(hipMemcpyAsync(d_out, canary, nbuf, hipMemcpyHostToDevice, st));
            OK(gsasr_splat_forward_u8(&d, ws, bytes, d_out, ROWS, COLS, pitch, flags, st));
            CK(hipStreamSynchronize(st));
            CK(hipMemcpy(img, d_img, sizeof(float) * 3 * H * W, hipMemcpyDeviceToHost));
            CK(hipMemcpy(out, d_out, nbuf, hipMemcpyDeviceToHost));
            long wrong = 0, touched = 0, levels[256] = {0};
            float lo = 0.f, hi = 0.f;
            for (size_t i = 0; i < nbuf; ++i) {
                const size_t y = i / pitch, b = i % pitch;
                if (y < ROWS && b < 3 * COLS) {
                    const int x = (int)(b / 3), k = (int)(b % 3), kc = flags ? 2 - k : k;
                    const float val = img[((size_t)y * W + x) * 3 + kc];
                    const unsigned char q = (unsigned char)rintf(fminf(fmaxf(val, 0.f), 1.f) * 255.0f);
                    lo = fminf(lo, val); hi = fmaxf(hi, val);
                    ++levels[q];
                    if (out[i] != q) ++wrong;
                } else if (out[i] != canary[i]) ++touched;
            }
            int nlev = 0;
            for (int l = 0; l < 256; ++l) nlev += levels[l] != 0;
            printf("u8 forward dmax=%g flags=%u: %ld wrong bytes, %ld bytes outside the crop touched, %d levels, float image in [%g, %g]\n",
                   dmaxs[v], flags, wrong, touched, nlev, lo, hi);
            if (wrong || touched || nlev < 200 || !(lo < 0.f) || !(hi > 1.f)) bad = 1;
        }
        /* argument errors: status + message, nothing enqueued */
        if (gsasr_splat_forward_u8(&d, ws, bytes, d_out, 0, COLS, pitch, 0u, st) != GSASR_ERR_ARG) { printf("crop_rows 0 accepted\n"); bad = 1; }
        if (gsasr_splat_forward_u8(&d, ws, bytes, d_out, H + 1, COLS, pitch, 0u, st) != GSASR_ERR_ARG) { printf("crop taller than the grid accepted\n"); bad = 1; }
        if (gsasr_splat_forward_u8(&d, ws, bytes, d_out, ROWS, W + 1, 3 * (W + 1), 0u, st) != GSASR_ERR_ARG) { printf("crop wider than the grid accepted\n"); bad = 1; }
        if (gsasr_splat_forward_u8(&d, ws, bytes, d_out, ROWS, COLS, 3 * COLS - 1, 0u, st) != GSASR_ERR_ARG) { printf("short pitch accepted\n"); bad = 1; }
        if (gsasr_splat_forward_u8(&d, ws, bytes, NULL, ROWS, COLS, pitch, 0u, st) != GSASR_ERR_ARG) { printf("null out accepted\n"); bad = 1; }
        if (gsasr_splat_forward_u8(&d, ws, bytes, d_out, ROWS, COLS, pitch, 2u, st) != GSASR_ERR_ARG) { printf("unknown flag accepted\n"); bad = 1; }
        if (!strlen(gsasr_last_error())) { printf("no error message\n"); bad = 1; }
        CK(hipFree(ws));
    }
    if (gsasr_abi_version() != 7) { printf("ABI version changed\n"); bad = 1; }
    printf("%s\n", bad ? "C-ABI U8 CHECK FAILED" : "C-ABI U8 CHECK OK");
    return bad;
}
