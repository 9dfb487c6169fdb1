// mfma_f32_layout_check.hip -- the operand and result lane maps of v_mfma_f32_16x16x4_f32 that csrc/splat_attn.hip relies on, checked
// with exact integer data and ASYMMETRIC operands (a symmetric one passes a kernel whose rows and columns are swapped):
//     lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; it receives D[row 4 (l >> 4) + reg][col l & 15].
// Also the chained form of the attention kernels: a result tile used in place as the next product's A operand, with the MFMA's
// k index g read as the tile's row 4 g + r.
//     hipcc --offload-arch=gfx950 -O2 tools/mfma_f32_layout_check.hip -o tools/bin/mfma_f32_layout_check && tools/bin/mfma_f32_layout_check
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

typedef float f4 __attribute__((ext_vector_type(4)));

// out[0..255] = D = A B with A[16][4], B[4][16]; out[256..511] = E = D^T-chain: E[m][n] = sum_x D[x][m] * V[x][n], V[16][16]
__global__ void k_check(const float *A, const float *B, const float *V, float *out)
{
    const int l = threadIdx.x, c = l & 15, g = l >> 4;
    f4 d = {0.f, 0.f, 0.f, 0.f};
    d = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c * 4 + g], B[g * 16 + c], d, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[(4 * g + r) * 16 + c] = d[r];
    // the lane holds D[4 g + r][c]: as the A operand A'[row c][k = g] of step r it stands for D^T[c][x = 4 g + r]
    f4 e = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 4; ++r) e = __builtin_amdgcn_mfma_f32_16x16x4f32(d[r], V[(4 * g + r) * 16 + c], e, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[256 + (4 * g + r) * 16 + c] = e[r];
}

#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main()
{
    float A[64], B[64], V[256], D[256], E[256], got[512];
    for (int i = 0; i < 16; ++i) for (int k = 0; k < 4; ++k) A[i * 4 + k] = (float)(1 + i + 2 * k * k);      // asymmetric; every sum below is exact in fp32
    for (int k = 0; k < 4; ++k) for (int j = 0; j < 16; ++j) B[k * 16 + j] = (float)(2 + k + (j * j) % 7);
    for (int x = 0; x < 16; ++x) for (int n = 0; n < 16; ++n) V[x * 16 + n] = (float)(1 + (2 * x + 3 * n + x * n) % 7);
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 16 + j];
        D[i * 16 + j] = s;
    }
    for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) {
        float s = 0.f;
        for (int x = 0; x < 16; ++x) s += D[x * 16 + m] * V[x * 16 + n];
        E[m * 16 + n] = s;
    }
    float *dA, *dB, *dV, *dO;
    TRY(hipMalloc(&dA, sizeof A)); TRY(hipMalloc(&dB, sizeof B)); TRY(hipMalloc(&dV, sizeof V)); TRY(hipMalloc(&dO, sizeof got));
    TRY(hipMemcpy(dA, A, sizeof A, hipMemcpyHostToDevice)); TRY(hipMemcpy(dB, B, sizeof B, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dV, V, sizeof V, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_check, dim3(1), dim3(64), 0, 0, dA, dB, dV, dO);
    TRY(hipGetLastError());
    TRY(hipMemcpy(got, dO, sizeof got, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < 256; ++i) bad += (got[i] != D[i]) + (got[256 + i] != E[i]);
    printf("mfma_f32_16x16x4f32 operand / result maps and the in-place chain: %s (%d of 512 values differ)\n", bad ? "WRONG" : "ok", bad);
    return bad ? 1 : 0;
}
