// mfma_f32_layout_check.hip -- the operand and result lane maps of v_mfma_f32_16x16x4_f32 that csrc/splat_attn.hip relies on, checked
// with exact integer data and ASYMMETRIC operands (a symmetric one passes a kernel whose rows and columns are swapped):
//     lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; it receives D[row 4 (l >> 4) + reg][col l & 15].
// Also the chained form of the attention kernels: a result tile used in place as the next product's A operand, with the MFMA's
// k index g read as the tile's row 4 g + r.
// And the bf16 shape of the bf16 forward, v_mfma_f32_16x16x32_bf16:
//     lane l supplies A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7, and receives the same D map;
// chained, two result tiles X0, X1 (keys 0..15 and 16..31 on their rows) rounded to bf16 are ONE A operand whose element j of lane
// group g is key 16 (j >> 2) + 4 g + (j & 3): the B operand must be fetched in that permuted k order.
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

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// out[0..511] = the two tiles D_t = A_t B (A_t [16][32] = rows 16 t .. of A, B [32][16]); out[512..767] = E[m][n] =
// sum over x < 32 of D[x][m] V[x][n] with D = (D_0; D_1) [32][16] and V [32][16], the permuted-k chain
__global__ void k_check_bf16(const float *A, const float *B, const float *V, float *out)
{
    const int l = threadIdx.x, c = l & 15, g = l >> 4;
    bf8 b, pf, vf;
    for (int j = 0; j < 8; ++j) b[j] = (__bf16)B[(8 * g + j) * 16 + c];
    f4 d[2];
    for (int t = 0; t < 2; ++t) {
        bf8 a;
        for (int j = 0; j < 8; ++j) a[j] = (__bf16)A[(16 * t + c) * 32 + 8 * g + j];
        const f4 zero = {0.f, 0.f, 0.f, 0.f};
        d[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, zero, 0, 0, 0);
        for (int r = 0; r < 4; ++r) out[256 * t + (4 * g + r) * 16 + c] = d[t][r];
    }
    // the lane holds D[16 t + 4 g + r][c]: as element j = 4 t + r of the A operand's row c it stands for x = 16 (j >> 2) + 4 g + (j & 3)
    for (int j = 0; j < 8; ++j) {
        pf[j] = (__bf16)d[j >> 2][j & 3];
        vf[j] = (__bf16)V[(16 * (j >> 2) + 4 * g + (j & 3)) * 16 + c];
    }
    f4 e = {0.f, 0.f, 0.f, 0.f};
    e = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, e, 0, 0, 0);
    for (int r = 0; r < 4; ++r) out[512 + (4 * g + r) * 16 + c] = e[r];
}

#define TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

static int check_bf16()
{
    static float A[32 * 32], B[32 * 16], V[32 * 16], D[32 * 16], E[256], got[768];
    // asymmetric; every operand and every D is an integer below 256 (exact in bf16), every sum exact in fp32
    for (int i = 0; i < 32; ++i) for (int k = 0; k < 32; ++k) A[i * 32 + k] = (float)((i + 2 * k + i * k) % 3);
    for (int k = 0; k < 32; ++k) for (int j = 0; j < 16; ++j) B[k * 16 + j] = (float)((3 * k + j * j + k * j) % 4);
    for (int x = 0; x < 32; ++x) for (int n = 0; n < 16; ++n) V[x * 16 + n] = (float)(1 + (2 * x + 3 * n + x * n) % 7);
    for (int i = 0; i < 32; ++i) for (int j = 0; j < 16; ++j) {
        float s = 0.f;
        for (int k = 0; k < 32; ++k) s += A[i * 32 + k] * B[k * 16 + j];
        D[i * 16 + j] = s;
    }
    for (int m = 0; m < 16; ++m) for (int n = 0; n < 16; ++n) {
        float s = 0.f;
        for (int x = 0; x < 32; ++x) s += D[x * 16 + m] * V[x * 16 + n];
        E[m * 16 + n] = s;
    }
    float *dA, *dB, *dV, *dO;
    TRY(hipMalloc(&dA, sizeof A)); TRY(hipMalloc(&dB, sizeof B)); TRY(hipMalloc(&dV, sizeof V)); TRY(hipMalloc(&dO, sizeof got));
    TRY(hipMemcpy(dA, A, sizeof A, hipMemcpyHostToDevice)); TRY(hipMemcpy(dB, B, sizeof B, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dV, V, sizeof V, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_check_bf16, dim3(1), dim3(64), 0, 0, dA, dB, dV, dO);
    TRY(hipGetLastError());
    TRY(hipMemcpy(got, dO, sizeof got, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < 512; ++i) bad += got[i] != D[i];
    for (int i = 0; i < 256; ++i) bad += got[512 + i] != E[i];
    printf("mfma_f32_16x16x32_bf16 operand / result maps and the permuted-k in-place chain: %s (%d of 768 values differ)\n", bad ? "WRONG" : "ok", bad);
    return bad ? 1 : 0;
}

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
    const int bad_bf16 = check_bf16();
    return bad ? 1 : bad_bf16;
}
