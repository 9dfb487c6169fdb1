// splat_attn.hip -- the window attention of GSASR's Fea2GS decoder (WindowCrossAttn / GSSelfAttn, utils/fea2gs.py:162-194, 321-350)
// as fused kernels: per window w and head h
//     out[w, :, h] = softmax(scale q[w, :, h] k[w, :, h]^T + table[index, h]) v[w, :, h]
// with q, k, v and out in the interleaved [windows, tokens, heads * head_dim] layout the Linears produce, and its gradient in
// q, k, v and the table: gsasr_window_attn_forward / _backward (one translation unit of libgsasr_splat.so; include/gsasr_splat.h
// has the contract).
//
// All products run on the exact-fp32 MFMA v_mfma_f32_16x16x4_f32 (lane l supplies A[row l & 15][k = l >> 4] and
// B[k = l >> 4][col l & 15]; it receives D[row 4 (l >> 4) + reg][col l & 15], reg = 0..3).  The head's slice of a window is
// zero-padded to 32 columns in LDS rows of 36 floats: the 4 x 16 reads of a B operand (row 4 (l >> 4) + r, column l & 15) are
// conflict-free, the 16 x 4 reads of an A operand (row l & 15, column 4 s + (l >> 4)) collide two by two on ds_read_b32's 32 banks
// (DESIGN.md 3.2i has the counters and the 8-byte form that would not).  The head's column of the table is staged in LDS as
// well (tables up to ATT_TAB_LDS rows), so a bias is an LDS read behind one 16-byte load of four indices.
//
//   k_attn_fwd     one workgroup (4 waves; 3 when the query tiles divide by 3 and not by 4) per (window, head), K and V in LDS.
//                  A wave takes 16 queries at a time and computes
//                  S^T = K (scale Q)^T: the lane then holds, for ITS query l & 15, the keys 16 t + 4 (l >> 4) + r of every key
//                  tile t -- the whole score row is in the registers of four lanes, so the softmax is exact (one maximum, one
//                  sum, two xor shuffles each), the bias is gathered from table[index[i, j], h] into the same registers, and
//                  P is already the A operand of O = P V when the MFMA's k index g is read as key 16 t + 4 g + r (V's rows
//                  are fetched in that order): no score leaves the registers.  Optional row statistic log-sum-exp.
//   k_attn_bwd_q   same geometry; P recomputed from the statistic, dP^T = V dO^T, dS = P (dP - delta) with
//                  delta = rowsum(dO o O), dq = scale dS K with dS as the A operand in place.  d table: dS is binned with LDS
//                  float adds into the workgroup's copy of the head's table column; a workgroup walks the windows
//                  b, b + stride, ... of its head and writes ONE partial column at the end (k_attn_table_sum adds the
//                  partials in a fixed order).  Tables above ATT_TAB_LDS rows: global atomics in DOUBLE on a zeroed column
//                  in the scratch, rounded to g_table once by k_attn_table_round (a row's sum has windows x pairs terms
//                  in no fixed order: in fp32 its error grew with the root of that count, past the fp32 torch sum's).
//   k_attn_bwd_kv  one workgroup per (window, head) with scale Q, dO, the statistic and delta in LDS; a wave takes 16 KEYS at a
//                  time and computes S = (scale Q) K^T and dP = dO V^T with the key on the lane: P^T and dS^T are then the A
//                  operands of dv = P^T dO and dk = dS^T (scale Q) in place.
// Every workgroup owns its window-head whole: dq, dk, dv are written once, without atomics, and two runs give the same bits.
// Both backward kernels form S exactly as the forward did (same chain, then the bias): the statistic is of those bits.
// The table gradient depends on the order of the LDS float adds.
//
// The rotary variant (gsasr_window_attn_rope_forward / _backward: the RoPE decoder of utils/fea2gsropeamp.py) is the same three
// kernels with ROPE = true: no table, no index, no bias; q and k rotated by the angles' (cos, sin), which k_attn_cossin writes
// once per call.  K (or scale Q in k_attn_bwd_kv) is rotated as it is staged, the row kept in registers as it is loaded, every
// value through att_rot and "rotate, then scale", so that S has the forward's bits in all three; dq and dk are multiplied by the
// conjugate at the store (the pair's other column is on lane ^ 1 of the D layout).  The angle gradient is a sum over windows of
// Im(conj(x) g_x) of the un-rotated q, k and their gradients: k_attn_angle_grad (a slice of windows per thread, in window
// order) and k_attn_angle_sum (the slices in order) -- fixed order, no atomics, the same bits in every run.
//
// The bf16 entry points (gsasr_window_attn_bf16_* / gsasr_window_attn_rope_bf16_*: q, k, v, out and their gradients bf16 in
// memory, everything else fp32; include/gsasr_splat.h has the numerical contract).  Forward: k_attn_fwd_bf, the geometry of
// k_attn_fwd on v_mfma_f32_16x16x32_bf16 -- one instruction per score tile, V staged transposed for the permuted k order of P.
// Backward: the kernels above instantiated on the element type T = att_bf (loads widen, stores round to nearest even, the
// rotated operands are rounded to bf16 where they are formed); the products stay on the exact-fp32 instruction.
//
// The masked family (gsasr_window_attn_masked / _masked_bf16: the attention of a Swin layer, utils/swinir.py:226-257) is the
// biased kernels with MK = true: S = (scale q k^T + B) + mask[w % mask_windows] in that order, the row's mask values loaded with
// its biases (k_attn_fwd: the whole row up front; the backward kernels: one tile ahead, in k_attn_bwd_kv down the lane's key
// column), and q, k, v, g_q, g_k, g_v each at its own row pitch, so that a packed [windows, n, 3 C] tensor is read and its
// gradient written in place.  MK kernels take AttnArgsMT (AttnArgsT plus the mask and the pitches); with MK = false every
// expression is the one it was, and the other families' kernels keep their instruction streams.
//
// The host layer is written once for the six descriptor types.  AttnFamily<descriptor> (AttnBiased, AttnRotary or AttnMasked on
// float or att_bf) states what differs: the required pointers, the alignment rule, the head_dim and table_rows / angle_rows
// rules, the scratch, each with its message, the kernels' argument type and the family's fields of it.  attn_check, attn_args,
// attn_forward and attn_backward are templates on the descriptor and the eighteen extern "C" functions one call each; a new
// variant is a family and its three entry points.  att_pick turns the runtime (key tiles -> MAXT 3 / 9 / 16, the masked family 3 / 4 / 9 / 16; stats, table in LDS, TAB) into template arguments;
// the dynamic LDS of a kernel is one struct (AttLdsQ, AttLdsKV, AttLdsFwdBf) that the kernel walks to its pointers and the
// host asks for the byte count.  The four kernels that touch no activation take AttnAux and exist once.
#include "splat_common.h"

#include <algorithm>
#include <initializer_list>
#include <type_traits>

using namespace gsasr_detail;

namespace {

typedef float att_f4 __attribute__((ext_vector_type(4)));

constexpr int ATT_LD = 36;            // floats per LDS row (32 columns + 4: see above)
constexpr int ATT_MAX_N = 256;        // tokens per window, queries or keys
constexpr int ATT_MAX_D = 32;         // head dimension
constexpr int ATT_TAB_LDS = 4096;     // table rows up to which d table is binned in LDS
constexpr int ATT_TAB_WG = 256;       // window slots (workgroups per head) of k_attn_bwd_q = partial columns per head, at most

typedef unsigned short att_bf;        // a bf16 in memory (gsasr_bf16)

// T = the activations' element type: float, or att_bf for the bf16 entry points (the table, the angles, the statistic, the
// (cos, sin) table and their gradients are fp32 in both)
template <typename T>
struct AttnArgsT {
    const T *q, *k, *v;
    const float *table;
    const T *out, *grad_out;
    const int *index;
    T *o;
    float *stats;
    T *g_q, *g_k, *g_v;
    float *g_table, *part;
    int windows, heads, nq, nk, d, rows, wslots;
    bool vec;       // index rows can be read 16 bytes at a time
    float scale;
    // the rotary variant (ROPE kernels; no table, no index)
    const float *angles;
    float *cossin, *g_angles;
    int arows, achunk, aslices;     // angle rows; windows per slice and slices of the angle gradient's first stage
    int ldvec;      // bf16 forward: elements per global load of q, k, v (8, 2 or 1: the head's slice is 16-, 4- or 2-byte aligned)
};
typedef AttnArgsT<float> AttnArgs;

// the arguments of the masked family's kernels (MK): the other families' kernels keep AttnArgsT, and with it their code
template <typename T>
struct AttnArgsMT : AttnArgsT<T> {
    const float *mask;      // [mwin, nq, nk], window w reads mask[w % mwin]; null: no mask
    int mwin;               // (at least 1, so that w % mwin is defined without a mask)
    bool mvec;              // mask rows can be read 16 bytes at a time
    int pq, pk, pv, pgq, pgk, pgv;      // elements between consecutive rows of q, k, v and of g_q, g_k, g_v
};
template <typename T, bool MK> using AttArgs = std::conditional_t<MK, AttnArgsMT<T>, AttnArgsT<T>>;

// what a kernel reads of them (the plain arguments: the contiguous pitch C everywhere and no mask)
struct AttPitch { int q, k, v, gq, gk, gv; };
struct AttMask { const float *p; int win; bool vec; };
#define ATT_MASKED_ARGS(A, C) \
    AttPitch P = {C, C, C, C, C, C}; \
    AttMask M = {nullptr, 1, false}; \
    if constexpr (MK) { P = {A.pq, A.pk, A.pv, A.pgq, A.pgk, A.pgv}; M = {A.mask, A.mwin, A.mvec}; }

// what the kernels that touch no activation read (k_attn_table_sum, k_attn_table_round, k_attn_cossin, k_attn_angle_sum)
// (no two integers that one of them reads lie side by side unless they did in AttnArgsT: each kernel keeps its scalar loads)
struct AttnAux {
    float *g_table, *part; int heads; const float *angles; float *cossin; int d; float *g_angles;
    int arows, rows, wslots, aslices;
};

// The dynamic LDS of an activation kernel is described in ONE place: a struct with the sizes of its sub-buffers in the order
// they lie in, and their sum.  The kernel walks the sizes to its pointers, the host launches with bytes().
// k_attn_fwd and k_attn_bwd_q, in floats: K and V (`kv` each: [keys padded to tiles][ATT_LD]), the head's table column (`tb`:
// the table's rows with TLDS, else 0), the binned table gradient (`tab`: the rows with TAB 1, else 0)
struct AttLdsQ {
    int kv, tb, tab;
    __host__ __device__ AttLdsQ(int nk, int tb_rows, int tab_rows = 0) : kv((((nk + 15) >> 4) << 4) * ATT_LD), tb(tb_rows), tab(tab_rows) {}
    __host__ size_t bytes() const { return ((size_t)kv + kv + tb + tab) * sizeof(float); }
};

// k_attn_bwd_kv, in floats: scale Q and dO (`qg` each: [queries padded to tiles][ATT_LD]), the statistic and delta (`nqp` each),
// the table column (`tb`)
struct AttLdsKV {
    int nqp, qg, tb;
    __host__ __device__ AttLdsKV(int nq, int tb_rows) : nqp(((nq + 15) >> 4) << 4), qg(nqp * ATT_LD), tb(tb_rows) {}
    __host__ size_t bytes() const { return ((size_t)qg + qg + nqp + nqp + tb) * sizeof(float); }
};

// one activation as fp32, a column pair as fp32, and the store: bf16 widens exactly and is rounded to nearest even at the store
__device__ __forceinline__ float att_ld(const float *p) { return *p; }
__device__ __forceinline__ float att_ld(const att_bf *p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ float2 att_ld2(const float *p) { return *reinterpret_cast<const float2 *>(p); }
__device__ __forceinline__ float2 att_ld2(const att_bf *p)
{
    const unsigned u = *reinterpret_cast<const unsigned *>(p);
    return make_float2(__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u));
}
__device__ __forceinline__ att_bf att_bits(float x) { return __builtin_bit_cast(att_bf, (__bf16)x); }
__device__ __forceinline__ void att_st(float *p, float x) { *p = x; }
__device__ __forceinline__ void att_st(att_bf *p, float x) { *p = att_bits(x); }
// a rotated operand as the products see it: the bf16 ops round it to bf16 (the reference rotates x.float() and returns type_as(x))
template <typename T> __device__ __forceinline__ float att_rnd(float x) { return x; }
template <> __device__ __forceinline__ float att_rnd<att_bf>(float x) { return (float)(__bf16)x; }

__device__ __forceinline__ att_f4 att_mfma(float a, float b, att_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// rows [0, n) x columns [0, d) of the head's slice of `src` (row pitch C floats) times `mul` into s[rows_pad][ATT_LD], zero elsewhere
template <typename T>
__device__ __forceinline__ void att_stage(float *s, const T *__restrict__ src, int n, int rows_pad, int d, int C, float mul)
{
    // eight loads in flight per thread before the first LDS store (one load per round trip made the staging the kernels' largest cost)
    const int nthr = blockDim.x;      // (a multiple of 64)
    for (int e0 = threadIdx.x; e0 < rows_pad * 32; e0 += 8 * nthr) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + nthr * u, j = e >> 5, c = e & 31;
            x[u] = (j < n && c < d) ? att_ld(src + (size_t)j * C + c) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + nthr * u;
            if (e < rows_pad * 32) s[(e >> 5) * ATT_LD + (e & 31)] = x[u] * mul;
        }
    }
}

// head h's column of the table into LDS (TLDS kernels: table_rows <= ATT_TAB_LDS), so that a bias is an LDS read
template <typename T>
__device__ __forceinline__ void att_stage_table(float *s_tb, const AttnArgsT<T> &A, int h)
{
    for (int t = threadIdx.x; t < A.rows; t += blockDim.x) s_tb[t] = A.table[(size_t)t * A.heads + h];
}

template <bool TLDS>
__device__ __forceinline__ float att_bias(const float *s_tb, const float *__restrict__ table, int heads, int h, int ix)
{
    return TLDS ? s_tb[ix] : table[(size_t)ix * heads + h];
}

// index[row][j0 .. j0 + 3] with j0 a multiple of 4; entries past nk repeat a valid one (their scores are masked).  `vec`: nk is a
// multiple of 4 and the array 16-byte aligned -- one 16-byte load.  Always unconditional: loads under a lane mask are not batched
__device__ __forceinline__ void att_load_index(int (&ix)[4], const int *__restrict__ irow, int j0, int nk, bool vec)
{
    if (vec) {
        const int4 v = *reinterpret_cast<const int4 *>(irow + min(j0, nk - 4));
        ix[0] = v.x; ix[1] = v.y; ix[2] = v.z; ix[3] = v.w;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) ix[r] = irow[min(j0 + r, nk - 1)];
    }
}

// mask[row][j0 .. j0 + 3] as att_load_index reads the index: entries past nk repeat a valid one, `vec` is one 16-byte load
__device__ __forceinline__ void att_load_mask(att_f4 &m, const float *__restrict__ mrow, int j0, int nk, bool vec)
{
    if (vec) m = *reinterpret_cast<const att_f4 *>(mrow + min(j0, nk - 4));
    else {
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = mrow[min(j0 + r, nk - 1)];
    }
}

// exp(x) as v_exp_f32(x log2 e): the rounding of the product moves p by at most |x| 2^-24 p <= 2.2e-8 (|x| e^-|x| peaks at 1)
__device__ __forceinline__ float att_exp(float x) { return __expf(x); }

// the sum / maximum over the four lanes l, l ^ 16, l ^ 32, l ^ 48 (one score row)
__device__ __forceinline__ float att_row_sum(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }
__device__ __forceinline__ float att_row_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); return fmaxf(v, __shfl_xor(v, 32)); }

// the eight A / B values of a row-operand kept in registers: x[row][4 s + g], s = 0..7 (0 past d columns or when !valid)
template <typename T>
__device__ __forceinline__ void att_load_row(float (&r)[8], const T *__restrict__ row, int g, int d, bool valid, float mul)
{
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int c = 4 * s + g;
        r[s] = (valid && c < d) ? att_ld(row + c) * mul : 0.f;
    }
}

// Rotary variant: column pair (2 j, 2 j + 1) of a token at angle row n is the complex number re + i im times cos + i sin of
// angles[h, n, j].  One component: x its own column, xp the pair's other column, odd = the imaginary one.  EVERY kernel forms
// a rotated value through this function and then multiplies by `mul`, so that forward and backward see the same bits; with
// (cs, -sn) it is the conjugate (the gradient of the un-rotated input from that of the rotated one: a rotation is unitary)
__device__ __forceinline__ float att_rot(float x, float xp, float cs, float sn, bool odd) { return fmaf(x, cs, xp * (odd ? sn : -sn)); }

// att_stage with the rows rotated: `cs` = the head's (cos, sin) rows [angle_rows][d / 2].  The pair's other column is on the
// neighbouring lane (element e = 32 row + column, consecutive over the lanes)
template <typename T>
__device__ __forceinline__ void att_stage_rot(float *s, const T *__restrict__ src, const float2 *__restrict__ cs, int n, int rows_pad, int d, int C, float mul)
{
    const int nthr = blockDim.x, hd = d >> 1;
    for (int e0 = threadIdx.x; e0 < rows_pad * 32; e0 += 8 * nthr) {
        float x[8];
        float2 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + nthr * u, j = e >> 5, c = e & 31;
            const bool ok = j < n && c < d;
            x[u] = ok ? att_ld(src + (size_t)j * C + c) : 0.f;
            t[u] = ok ? cs[j * hd + (c >> 1)] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + nthr * u;
            const float xp = __shfl_xor(x[u], 1);       // (whole waves get here: rows_pad * 32 and nthr are multiples of 64)
            if (e < rows_pad * 32) s[(e >> 5) * ATT_LD + (e & 31)] = att_rnd<T>(att_rot(x[u], xp, t[u].x, t[u].y, e & 1)) * mul;
        }
    }
}

// att_load_row with the row rotated by its (cos, sin) row `cs` [d / 2]: both columns of a pair in one 8-byte load
template <typename T>
__device__ __forceinline__ void att_load_row_rot(float (&r)[8], const T *__restrict__ row, const float2 *__restrict__ cs, int g, int d, bool valid, float mul)
{
    const bool odd = g & 1;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int c = 4 * s + g, pj = c >> 1;
        const bool ok = valid && c < d;
        const float2 xy = ok ? att_ld2(row + 2 * pj) : make_float2(0.f, 0.f);
        const float2 t = ok ? cs[pj] : make_float2(0.f, 0.f);
        r[s] = att_rnd<T>(att_rot(odd ? xy.y : xy.x, odd ? xy.x : xy.y, t.x, t.y, odd)) * mul;
    }
}

// the D tile's value `a` (row of angle row `n`, column c16 + 16 * half) times the conjugate: its pair's other column is on lane ^ 1
__device__ __forceinline__ float att_unrot(float a, const float2 *__restrict__ cs, int n, int hd, int col, int d)
{
    const float xp = __shfl_xor(a, 1);
    const float2 t = col < d ? cs[n * hd + (col >> 1)] : make_float2(0.f, 0.f);
    return att_rot(a, xp, t.x, -t.y, col & 1);
}

// D = sum_s A_lds[row0 + (l & 15)][4 s + g] * b[s]: a 16 x 16 tile over the 32 padded columns
__device__ __forceinline__ att_f4 att_tile(const float *s_a, int row0, int c16, int g, const float (&b)[8])
{
    att_f4 acc = {0.f, 0.f, 0.f, 0.f};
    const float *p = s_a + (row0 + c16) * ATT_LD + g;
    float a[8];         // (all eight reads before the first product: a product that waits for its own LDS read runs at LDS latency)
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = p[4 * s];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = att_mfma(a[s], b[s], acc);
    return acc;
}

// the thread's place in its workgroup and in the MFMA layouts: {wave, waves, c16 = lane & 15, g = lane >> 4}
struct AttLane { int wave, nwaves, c16, g; };
__device__ __forceinline__ AttLane att_lane() { return {(int)(threadIdx.x >> 6), (int)(blockDim.x >> 6), (int)(threadIdx.x & 15), (int)(threadIdx.x & 63) >> 4}; }

// the backward kernels' index pipeline, two tiles ahead: this tile's index <- the next tile's <- the one just loaded
__device__ __forceinline__ void att_shift(int &ix, int &ix1, int ixn) { ix = ix1; ix1 = ixn; }

// ROPE: q and k rotated (K as it is staged, the query row in registers; rotate, then scale), no table / index / bias
// MK (the masked family): S = (scale q k^T + B) + mask[w % mwin], the row's mask values loaded with its biases (a uniform branch
// around the loads when the call has no mask: + 0 then), and q, k, v read at their own row pitches
template <int MAXT, bool STATS, bool TLDS, bool ROPE = false, bool MK = false>
__global__ __launch_bounds__(256) void k_attn_fwd(AttArgs<float, MK> A)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int w = blockIdx.x / A.heads, h = blockIdx.x % A.heads;
    const int nq = A.nq, nk = A.nk, d = A.d, C = A.heads * A.d;
    ATT_MASKED_ARGS(A, C)
    const int Cq = P.q, Ck = P.k, Cv = P.v;
    const int nt = (nk + 15) >> 4, nkp = nt << 4;
    const AttLdsQ L(nk, TLDS ? A.rows : 0);
    float *s_k = s_mem, *s_v = s_k + L.kv, *s_tb = s_v + L.kv;
    const float2 *cs = ROPE ? reinterpret_cast<const float2 *>(A.cossin) + (size_t)h * A.arows * (d >> 1) : nullptr;
    if (ROPE) att_stage_rot(s_k, A.k + (size_t)w * nk * Ck + h * d, cs, nk, nkp, d, Ck, 1.f);
    else att_stage(s_k, A.k + (size_t)w * nk * Ck + h * d, nk, nkp, d, Ck, 1.f);
    att_stage(s_v, A.v + (size_t)w * nk * Cv + h * d, nk, nkp, d, Cv, 1.f);
    if (TLDS) att_stage_table(s_tb, A, h);
    __syncthreads();
    const auto [wave, nwaves, c16, g] = att_lane();
    const int nqt = (nq + 15) >> 4;
    const float *mwin = MK && M.p ? M.p + (size_t)(w % M.win) * nq * nk : nullptr;
    for (int qt = wave; qt < nqt; qt += nwaves) {
        const int i = qt * 16 + c16, ic = min(i, nq - 1);       // (rows past nq repeat the last query and are not stored)
        float qr[8];
        if (ROPE) att_load_row_rot(qr, A.q + ((size_t)w * nq + ic) * Cq + h * d, cs + ic * (d >> 1), g, d, true, A.scale);
        else att_load_row(qr, A.q + ((size_t)w * nq + ic) * Cq + h * d, g, d, true, A.scale);
        att_f4 sc[MAXT];
        const int *irow = ROPE ? nullptr : A.index + (size_t)ic * nk;
        float m = -INFINITY;
        att_f4 bs[ROPE ? 1 : MAXT];         // (the whole row's biases first)
        att_f4 ms[MK ? MAXT : 1];           // (and its mask values)
        if (MK) {
#pragma unroll
            for (int t = 0; t < (MK ? MAXT : 0); ++t) ms[t] = att_f4{0.f, 0.f, 0.f, 0.f};
            if (mwin) {
#pragma unroll
                for (int t = 0; t < (MK ? MAXT : 0); ++t) att_load_mask(ms[t], mwin + (size_t)ic * nk, 16 * t + 4 * g, nk, M.vec);
            }
        }
#pragma unroll
        for (int t = 0; t < (ROPE ? 0 : MAXT); ++t) {
            int ix[4];
            att_load_index(ix, irow, 16 * t + 4 * g, nk, A.vec);
#pragma unroll
            for (int r = 0; r < 4; ++r) bs[t][r] = att_bias<TLDS>(s_tb, A.table, A.heads, h, ix[r]);
        }
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                sc[t] = att_tile(s_k, 16 * t, c16, g, qr);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[t][r] = 16 * t + 4 * g + r < nk ? (ROPE ? sc[t][r] : MK ? (sc[t][r] + bs[ROPE ? 0 : t][r]) + ms[MK ? t : 0][r] : sc[t][r] + bs[ROPE ? 0 : t][r]) : -INFINITY;
                    m = fmaxf(m, sc[t][r]);
                }
            }
        }
        m = att_row_max(m);
        float l = 0.f;
        att_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                const float *vr = s_v + (16 * t + 4 * g) * ATT_LD + c16;
                float v0[4], v1[4], p[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v0[r] = vr[r * ATT_LD];
                    v1[r] = vr[r * ATT_LD + 16];
                    p[r] = att_exp(sc[t][r] - m);
                    l += p[r];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    o0 = att_mfma(p[r], v0[r], o0);
                    o1 = att_mfma(p[r], v1[r], o1);       // (always: the padded columns are zero, and a branch per product blocks the scheduler)
                }
            }
        }
        l = att_row_sum(l);
        if (STATS && g == 0 && i < nq) A.stats[((size_t)w * A.heads + h) * nq + i] = m + logf(l);
        const float linv = 1.f / l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {       // the tile's row 4 g + r belongs to the query on lane 4 g + r
            const float f = __shfl(linv, 4 * g + r);
            const int io = qt * 16 + 4 * g + r;
            if (io < nq) {
                float *po = A.o + ((size_t)w * nq + io) * C + h * d;
                if (c16 < d) po[c16] = o0[r] * f;
                if (c16 + 16 < d) po[c16 + 16] = o1[r] * f;
            }
        }
    }
}

// ---- the forward of the bf16 ops, on v_mfma_f32_16x16x32_bf16 ----------------------------------------------------
// Lane l supplies A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7 (eight bf16 = 16 bytes), and
// receives D[row 4 (l >> 4) + reg][col l & 15] as above (tools/mfma_f32_layout_check.hip checks the maps).  The padded head
// dimension 32 is ONE k step: S^T = K Q^T is one instruction per key tile, its A operand one 16-byte LDS read of a K row, its
// B operand the query's eight consecutive columns, kept in registers.  P is the A operand of O = P V in place: a step takes the
// key tiles 2 u and 2 u + 1, element j of lane group g is key 32 u + 16 (j >> 2) + 4 g + (j & 3), so V is staged TRANSPOSED
// ([column][key], keys zero-filled to whole steps: an odd tile count leaves a half-empty step whose p are 0) and its B operand
// is two 8-byte reads of four consecutive keys.  LDS pitches: K rows of 40 bf16 = 20 words (the rows l & 15 of a 16-byte read
// start 20 r mod 64 banks apart, all different multiples of 4); V^T rows of keys + 8 bf16 = 16 m + 4 words (4 (4 m + 1) r mod 64:
// the sixteen columns of an 8-byte read land on different groups of four banks).
typedef __bf16 att_bf8 __attribute__((ext_vector_type(8)));
constexpr int ATT_KLD = 40;       // bf16 per LDS row of K
constexpr int ATT_VPAD = 8;       // bf16 past the padded keys per LDS row of V^T

__device__ __forceinline__ att_f4 att_mfma_bf(att_bf8 a, att_bf8 b, att_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ att_bf8 att_frag(unsigned a, unsigned b, unsigned c, unsigned d) { return __builtin_bit_cast(att_bf8, make_uint4(a, b, c, d)); }

// VEC consecutive bf16 at p as packed pairs (0 when !ok): one 16-, 4- or 2-byte load
template <int VEC>
__device__ __forceinline__ void att_ld_raw(unsigned (&w)[(VEC + 1) / 2], const att_bf *__restrict__ p, bool ok)
{
    if constexpr (VEC == 8) {
        const uint4 u = ok ? *reinterpret_cast<const uint4 *>(p) : make_uint4(0u, 0u, 0u, 0u);
        w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
    } else if constexpr (VEC == 2) w[0] = ok ? *reinterpret_cast<const unsigned *>(p) : 0u;
    else w[0] = ok ? (unsigned)*p : 0u;
}

// the packed pair (re, im) rotated by (cos, sin) in fp32, each component rounded to bf16
__device__ __forceinline__ unsigned att_rot_pair(unsigned w, float2 t)
{
    const float re = __uint_as_float(w << 16), im = __uint_as_float(w & 0xffff0000u);
    return (unsigned)att_bits(att_rot(re, im, t.x, t.y, false)) | ((unsigned)att_bits(att_rot(im, re, t.x, t.y, true)) << 16);
}

// the head's slices of K (rotated when ROPE) and V, rows [0, nk) x columns [0, d), into s_k[nkp32][ATT_KLD] and s_vt[32][vld],
// zero elsewhere.  U loads of K and of V in flight per thread before the first LDS store
template <int VEC, bool ROPE, bool MK = false>
__device__ __forceinline__ void att_stage_kv_bf(att_bf *s_k, att_bf *s_vt, const att_bf *__restrict__ ksrc, const att_bf *__restrict__ vsrc,
                                                const float2 *__restrict__ cs, int nk, int nkp32, int vld, int d, int Ck, int Cv)
{
    constexpr int CPR = 32 / VEC, NW = (VEC + 1) / 2, U = VEC == 8 ? 2 : 4;
    const int nthr = blockDim.x, total = nkp32 * CPR, hd = d >> 1;
    for (int e0 = threadIdx.x; e0 < total; e0 += U * nthr) {
        unsigned kw[U][NW], vw[U][NW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + nthr * u, j = e / CPR, cc = (e % CPR) * VEC;
            const bool ok = e < total && j < nk && cc < d;
            att_ld_raw<VEC>(kw[u], ksrc + (size_t)j * Ck + cc, ok);
            att_ld_raw<VEC>(vw[u], vsrc + (size_t)j * (MK ? Cv : Ck) + cc, ok);
            if constexpr (ROPE && VEC > 1) {
#pragma unroll
                for (int i = 0; i < NW; ++i) kw[u][i] = att_rot_pair(kw[u][i], ok ? cs[j * hd + (cc >> 1) + i] : make_float2(0.f, 0.f));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + nthr * u, j = e / CPR, cc = (e % CPR) * VEC;
            if (e < total) {
                att_bf *dk = s_k + j * ATT_KLD + cc;
                if constexpr (VEC == 8) *reinterpret_cast<uint4 *>(dk) = make_uint4(kw[u][0], kw[u][1], kw[u][2], kw[u][3]);
                else if constexpr (VEC == 2) *reinterpret_cast<unsigned *>(dk) = kw[u][0];
                else *dk = (att_bf)kw[u][0];
#pragma unroll
                for (int i = 0; i < VEC; ++i) s_vt[(cc + i) * vld + j] = (att_bf)(vw[u][i >> 1] >> (16 * (i & 1)));
            }
        }
    }
}

// the query's B fragment: columns 8 g .. 8 g + 7 of its row (0 past d), rotated by the row's (cos, sin) `cs` [d / 2] when ROPE
template <int VEC, bool ROPE>
__device__ __forceinline__ att_bf8 att_load_q_bf(const att_bf *__restrict__ row, const float2 *__restrict__ cs, int g, int d)
{
    unsigned w[4];
    if constexpr (VEC == 8) {
        const uint4 u = 8 * g < d ? *reinterpret_cast<const uint4 *>(row + 8 * g) : make_uint4(0u, 0u, 0u, 0u);
        w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 8 * g + 2 * i;
            if (VEC == 2) w[i] = c < d ? *reinterpret_cast<const unsigned *>(row + c) : 0u;
            else w[i] = (c < d ? (unsigned)row[c] : 0u) | (c + 1 < d ? (unsigned)row[c + 1] << 16 : 0u);
        }
    }
    if (ROPE) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = att_rot_pair(w[i], 8 * g + 2 * i < d ? cs[4 * g + i] : make_float2(0.f, 0.f));
    }
    return att_frag(w[0], w[1], w[2], w[3]);
}

// the dynamic LDS of k_attn_fwd_bf (as AttLdsQ): K (`k` bf16: [keys padded to paired steps of 32][ATT_KLD]), V transposed (`vt`
// bf16: [32][vld]), then the head's table column (`tb` floats)
struct AttLdsFwdBf {
    int nkp32, vld, k, vt, tb;
    __host__ __device__ AttLdsFwdBf(int nk, int tb_rows) : nkp32(((nk + 31) >> 5) << 5), vld(nkp32 + ATT_VPAD), k(nkp32 * ATT_KLD), vt(32 * vld), tb(tb_rows) {}
    __host__ size_t bytes() const { return ((size_t)k + vt) * sizeof(att_bf) + tb * sizeof(float); }
};

// The geometry of k_attn_fwd (one workgroup per (window, head), a wave takes 16 queries, the lane holds its query's whole score
// row in fp32: one maximum, one sum of the unrounded p).  scale multiplies the fp32 score sum; p is rounded to bf16 only as the
// operand of P V; out is rounded once at the store.  include/gsasr_splat.h has the contract.
template <int MAXT, bool STATS, bool TLDS, bool ROPE, bool MK = false>
__global__ __launch_bounds__(256) void k_attn_fwd_bf(AttArgs<att_bf, MK> A)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int w = blockIdx.x / A.heads, h = blockIdx.x % A.heads;
    const int nq = A.nq, nk = A.nk, d = A.d, C = A.heads * A.d;
    ATT_MASKED_ARGS(A, C)
    const int Cq = P.q, Ck = P.k, Cv = P.v;
    const int nt = (nk + 15) >> 4;
    const AttLdsFwdBf L(nk, TLDS ? A.rows : 0);
    const int nkp32 = L.nkp32, vld = L.vld;
    att_bf *s_k = reinterpret_cast<att_bf *>(s_mem), *s_vt = s_k + L.k;
    float *s_tb = reinterpret_cast<float *>(s_vt + L.vt);
    const float2 *cs = ROPE ? reinterpret_cast<const float2 *>(A.cossin) + (size_t)h * A.arows * (d >> 1) : nullptr;
    const att_bf *ksrc = A.k + (size_t)w * nk * Ck + h * d, *vsrc = A.v + (size_t)w * nk * Cv + h * d;
    if (A.ldvec == 8) att_stage_kv_bf<8, ROPE, MK>(s_k, s_vt, ksrc, vsrc, cs, nk, nkp32, vld, d, Ck, Cv);
    else if (A.ldvec == 2) att_stage_kv_bf<2, ROPE, MK>(s_k, s_vt, ksrc, vsrc, cs, nk, nkp32, vld, d, Ck, Cv);
    else if (!ROPE) att_stage_kv_bf<1, false, MK>(s_k, s_vt, ksrc, vsrc, cs, nk, nkp32, vld, d, Ck, Cv);
    if (TLDS) att_stage_table(s_tb, A, h);
    __syncthreads();
    const auto [wave, nwaves, c16, g] = att_lane();
    const int nqt = (nq + 15) >> 4;
    const float *mwin = MK && M.p ? M.p + (size_t)(w % M.win) * nq * nk : nullptr;
    for (int qt = wave; qt < nqt; qt += nwaves) {
        const int i = qt * 16 + c16, ic = min(i, nq - 1);       // (rows past nq repeat the last query and are not stored)
        const att_bf *qrow = A.q + ((size_t)w * nq + ic) * Cq + h * d;
        const float2 *qcs = ROPE ? cs + ic * (d >> 1) : nullptr;
        att_bf8 qf;
        if (A.ldvec == 8) qf = att_load_q_bf<8, ROPE>(qrow, qcs, g, d);
        else if (A.ldvec == 2) qf = att_load_q_bf<2, ROPE>(qrow, qcs, g, d);
        else qf = att_load_q_bf<1, false>(qrow, qcs, g, d);
        att_f4 sc[MAXT];
        const int *irow = ROPE ? nullptr : A.index + (size_t)ic * nk;
        float m = -INFINITY;
        att_f4 bs[ROPE ? 1 : MAXT];         // (the whole row's biases first)
        att_f4 ms[MK ? MAXT : 1];           // (and its mask values)
        if (MK) {
#pragma unroll
            for (int t = 0; t < (MK ? MAXT : 0); ++t) ms[t] = att_f4{0.f, 0.f, 0.f, 0.f};
            if (mwin) {
#pragma unroll
                for (int t = 0; t < (MK ? MAXT : 0); ++t) att_load_mask(ms[t], mwin + (size_t)ic * nk, 16 * t + 4 * g, nk, M.vec);
            }
        }
#pragma unroll
        for (int t = 0; t < (ROPE ? 0 : MAXT); ++t) {
            int ix[4];
            att_load_index(ix, irow, 16 * t + 4 * g, nk, A.vec);
#pragma unroll
            for (int r = 0; r < 4; ++r) bs[t][r] = att_bias<TLDS>(s_tb, A.table, A.heads, h, ix[r]);
        }
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (t < nt) {
                const att_bf8 kf = __builtin_bit_cast(att_bf8, *reinterpret_cast<const uint4 *>(s_k + (16 * t + c16) * ATT_KLD + 8 * g));
                const att_f4 zero = {0.f, 0.f, 0.f, 0.f};
                sc[t] = att_mfma_bf(kf, qf, zero);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = sc[t][r] * A.scale;         // (the fp32 sum times scale, then the fp32 bias)
                    sc[t][r] = 16 * t + 4 * g + r < nk ? (ROPE ? s : MK ? (s + bs[ROPE ? 0 : t][r]) + ms[MK ? t : 0][r] : s + bs[ROPE ? 0 : t][r]) : -INFINITY;
                    m = fmaxf(m, sc[t][r]);
                }
            }
        }
        m = att_row_max(m);
        float l = 0.f;
        att_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < (MAXT + 1) / 2; ++u) {
            if (2 * u < nt) {
                const att_bf *vr = s_vt + c16 * vld + 32 * u + 4 * g;
                const uint2 a0 = *reinterpret_cast<const uint2 *>(vr), a1 = *reinterpret_cast<const uint2 *>(vr + 16);
                const uint2 b0 = *reinterpret_cast<const uint2 *>(vr + 16 * vld), b1 = *reinterpret_cast<const uint2 *>(vr + 16 * vld + 16);
                float p[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = att_exp(sc[2 * u][r] - m);
                    p[4 + r] = (2 * u + 1 < MAXT && 2 * u + 1 < nt) ? att_exp(sc[2 * u + 1 < MAXT ? 2 * u + 1 : 0][r] - m) : 0.f;
                    l += p[r] + p[4 + r];
                }
                att_bf8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (__bf16)p[j];
                o0 = att_mfma_bf(pf, att_frag(a0.x, a0.y, a1.x, a1.y), o0);
                o1 = att_mfma_bf(pf, att_frag(b0.x, b0.y, b1.x, b1.y), o1);     // (always: the padded columns are zero)
            }
        }
        l = att_row_sum(l);
        if (STATS && g == 0 && i < nq) A.stats[((size_t)w * A.heads + h) * nq + i] = m + logf(l);
        const float linv = 1.f / l;
#pragma unroll
        for (int r = 0; r < 4; ++r) {       // the tile's row 4 g + r belongs to the query on lane 4 g + r
            const float f = __shfl(linv, 4 * g + r);
            const int io = qt * 16 + 4 * g + r;
            if (io < nq) {
                att_bf *po = A.o + ((size_t)w * nq + io) * C + h * d;
                if (c16 < d) po[c16] = att_bits(o0[r] * f);
                if (c16 + 16 < d) po[c16 + 16] = att_bits(o1[r] * f);
            }
        }
    }
}

// TAB: 0 no table gradient, 1 binned in LDS -> a partial column, 2 global double atomics on the scratch's [rows, heads]
// ROPE (TAB 0, no table): K staged rotated, the query row rotated in registers, dq times the conjugate at the store
// T: the activations' element type (bf16: loads widen as they stage, delta is of the bf16 out that was stored, dq is rounded at the store)
// MK: the mask of the window being walked (w, not the slot) joins S after the bias, one tile ahead; own pitches for q, k, v, g_q
template <int TAB, bool TLDS, bool ROPE = false, typename T = float, bool MK = false>
__global__ __launch_bounds__(256) void k_attn_bwd_q(AttArgs<T, MK> A)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int slot = blockIdx.x / A.heads, h = blockIdx.x % A.heads;
    const int nq = A.nq, nk = A.nk, d = A.d, C = A.heads * A.d;
    ATT_MASKED_ARGS(A, C)
    const int Cq = P.q, Ck = P.k, Cv = P.v, Cgq = P.gq;
    const int nt = (nk + 15) >> 4, nkp = nt << 4, nqt = (nq + 15) >> 4;
    const AttLdsQ L(nk, TLDS ? A.rows : 0, TAB == 1 ? A.rows : 0);
    float *s_k = s_mem, *s_v = s_k + L.kv, *s_tb = s_v + L.kv, *s_tab = s_tb + L.tb;
    const auto [wave, nwaves, c16, g] = att_lane();
    const float2 *cs = ROPE ? reinterpret_cast<const float2 *>(A.cossin) + (size_t)h * A.arows * (d >> 1) : nullptr;
    if (TAB == 1) for (int t = threadIdx.x; t < A.rows; t += blockDim.x) s_tab[t] = 0.f;
    if (TLDS) att_stage_table(s_tb, A, h);
    for (int w = slot; w < A.windows; w += A.wslots) {
        __syncthreads();        // (the previous window's reads of s_k / s_v are done; s_tab is zeroed)
        if (ROPE) att_stage_rot(s_k, A.k + (size_t)w * nk * Ck + h * d, cs, nk, nkp, d, Ck, 1.f);
        else att_stage(s_k, A.k + (size_t)w * nk * Ck + h * d, nk, nkp, d, Ck, 1.f);
        att_stage(s_v, A.v + (size_t)w * nk * Cv + h * d, nk, nkp, d, Cv, 1.f);
        __syncthreads();
        const float *mwin = MK && M.p ? M.p + (size_t)(w % M.win) * nq * nk : nullptr;
        for (int qt = wave; qt < nqt; qt += nwaves) {
            const int i = qt * 16 + c16, ic = min(i, nq - 1);
            const bool iv = i < nq;
            const size_t qoff = ((size_t)w * nq + ic) * C + h * d;
            float qr[8], gr[8], orow[8];
            const size_t qrow = MK ? ((size_t)w * nq + ic) * Cq + h * d : qoff;
            if (ROPE) att_load_row_rot(qr, A.q + qrow, cs + ic * (d >> 1), g, d, true, A.scale);
            else att_load_row(qr, A.q + qrow, g, d, true, A.scale);
            att_load_row(gr, A.grad_out + qoff, g, d, iv, 1.f);
            att_load_row(orow, A.out + qoff, g, d, iv, 1.f);
            float delta = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s) delta = fmaf(gr[s], orow[s], delta);
            delta = att_row_sum(delta);
            const float lse = A.stats[((size_t)w * A.heads + h) * nq + ic];
            const int *irow = ROPE ? nullptr : A.index + (size_t)ic * nk;
            att_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = {0.f, 0.f, 0.f, 0.f};
            // the tile's indices are loaded one tile ahead and its biases before its products: the dependent round trips run
            // under the MFMAs
            int ix[4], ix1[4];
            if (!ROPE) {
                att_load_index(ix, irow, 4 * g, nk, A.vec);
                att_load_index(ix1, irow, 16 + 4 * g, nk, A.vec);
            }
            att_f4 mk = {0.f, 0.f, 0.f, 0.f};       // (MK: this tile's mask values, the next tile's loaded under this one's products)
            if (MK && mwin) att_load_mask(mk, mwin + (size_t)ic * nk, 4 * g, nk, M.vec);
            for (int t = 0; t < nt; ++t) {
                float b[4];
                int ixn[4];     // (two tiles ahead: one tile's products are shorter than a round trip to L2)
                att_f4 mkn = {0.f, 0.f, 0.f, 0.f};
                if (MK && mwin) att_load_mask(mkn, mwin + (size_t)ic * nk, 16 * t + 16 + 4 * g, nk, M.vec);
                if (!ROPE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) b[r] = att_bias<TLDS>(s_tb, A.table, A.heads, h, ix[r]);
                    att_load_index(ixn, irow, 16 * t + 32 + 4 * g, nk, A.vec);
                }
                const float *kr = s_k + (16 * t + 4 * g) * ATT_LD + c16;
                float k0[4], k1[4], ds[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    k0[r] = kr[r * ATT_LD];
                    k1[r] = kr[r * ATT_LD + 16];
                }
                // (S exactly as the forward formed it -- the same chain, then the bias: the statistic is of THOSE bits, and at
                // scores of a few hundred one ulp of S is 3e-5 of P)
                const att_f4 sc = att_tile(s_k, 16 * t, c16, g, qr);
                const att_f4 dp = att_tile(s_v, 16 * t, c16, g, gr);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * t + 4 * g + r;
                    const bool valid = iv && j < nk;
                    const float p = valid ? att_exp((ROPE ? sc[r] : MK ? (sc[r] + b[r]) + mk[r] : sc[r] + b[r]) - lse) : 0.f;
                    ds[r] = p * (dp[r] - delta);
                    if (TAB == 1 && valid) atomicAdd(&s_tab[ix[r]], ds[r]);
                    if (TAB == 2 && valid) atomicAdd(reinterpret_cast<double *>(A.part) + (size_t)ix[r] * A.heads + h, (double)ds[r]);
                    att_shift(ix[r], ix1[r], ixn[r]);
                }
                if (MK) mk = mkn;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dq0 = att_mfma(ds[r], k0[r], dq0);
                    dq1 = att_mfma(ds[r], k1[r], dq1);
                }
            }
            if (A.g_q) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int io = qt * 16 + 4 * g + r;
                    float u0 = 0.f, u1 = 0.f;
                    if (ROPE) {         // (before the row's test: the shuffle wants the whole wave)
                        u0 = att_unrot(dq0[r] * A.scale, cs, min(io, nq - 1), d >> 1, c16, d);
                        u1 = att_unrot(dq1[r] * A.scale, cs, min(io, nq - 1), d >> 1, c16 + 16, d);
                    }
                    if (io < nq) {
                        T *po = A.g_q + ((size_t)w * nq + io) * Cgq + h * d;
                        if (c16 < d) att_st(po + c16, ROPE ? u0 : dq0[r] * A.scale);
                        if (c16 + 16 < d) att_st(po + c16 + 16, ROPE ? u1 : dq1[r] * A.scale);
                    }
                }
            }
        }
    }
    if (TAB == 1) {
        __syncthreads();
        float *part = A.part + ((size_t)slot * A.heads + h) * A.rows;
        for (int t = threadIdx.x; t < A.rows; t += blockDim.x) part[t] = s_tab[t];
    }
}

// g_table[t, h] = the partial columns of head h added in a fixed order: 32 entries per workgroup, eight threads per entry
// each adding the slots s = slice, slice + 8, ... (short chains of independent loads), then the eight sums in slice order
__global__ __launch_bounds__(256) void k_attn_table_sum(AttnAux A)
{
    __shared__ float s_sum[8][32];
    const int e = blockIdx.x * 32 + (threadIdx.x & 31), slice = threadIdx.x >> 5;
    const bool ev = e < A.rows * A.heads;
    const int h = ev ? e / A.rows : 0, t = ev ? e % A.rows : 0;
    float a = 0.f;
    if (ev) for (int s = slice; s < A.wslots; s += 8) a += A.part[((size_t)s * A.heads + h) * A.rows + t];
    s_sum[slice][threadIdx.x & 31] = a;
    __syncthreads();
    if (slice == 0 && ev) {
        for (int u = 1; u < 8; ++u) a += s_sum[u][threadIdx.x];
        A.g_table[(size_t)t * A.heads + h] = a;
    }
}

// g_table = the double sums of the TAB == 2 walk, rounded once
__global__ __launch_bounds__(256) void k_attn_table_round(AttnAux A)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < A.rows * A.heads) A.g_table[e] = (float)reinterpret_cast<const double *>(A.part)[e];
}

// ROPE: scale Q staged rotated, the key row rotated in registers, dk times the conjugate at the store
// MK: the mask column of the lane's key (mask[w % mwin][query][key]: the key is on the lane here), one tile ahead; own pitches
template <bool TLDS, bool ROPE = false, typename T = float, bool MK = false>
__global__ __launch_bounds__(256) void k_attn_bwd_kv(AttArgs<T, MK> A)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const int w = blockIdx.x / A.heads, h = blockIdx.x % A.heads;
    const int nq = A.nq, nk = A.nk, d = A.d, C = A.heads * A.d;
    ATT_MASKED_ARGS(A, C)
    const int Cq = P.q, Ck = P.k, Cv = P.v, Cgk = P.gk, Cgv = P.gv;
    const int nqt = (nq + 15) >> 4, nqp = nqt << 4, nkt = (nk + 15) >> 4;
    const AttLdsKV L(nq, TLDS ? A.rows : 0);
    float *s_q = s_mem, *s_g = s_q + L.qg, *s_lse = s_g + L.qg, *s_delta = s_lse + L.nqp, *s_tb = s_delta + L.nqp;
    const size_t qbase = (size_t)w * nq * C + h * d;
    const float2 *cs = ROPE ? reinterpret_cast<const float2 *>(A.cossin) + (size_t)h * A.arows * (d >> 1) : nullptr;
    const size_t qsrc = MK ? (size_t)w * nq * Cq + h * d : qbase;
    if (ROPE) att_stage_rot(s_q, A.q + qsrc, cs, nq, nqp, d, Cq, A.scale);
    else att_stage(s_q, A.q + qsrc, nq, nqp, d, Cq, A.scale);
    att_stage(s_g, A.grad_out + qbase, nq, nqp, d, C, 1.f);
    if (TLDS) att_stage_table(s_tb, A, h);
    __syncthreads();
    for (int i = threadIdx.x; i < nqp; i += blockDim.x) {
        float a = 0.f;
        if (i < nq) {
            const T *po = A.out + qbase + (size_t)i * C;
            for (int c = 0; c < d; ++c) a = fmaf(s_g[i * ATT_LD + c], att_ld(po + c), a);
        }
        s_delta[i] = a;
        s_lse[i] = i < nq ? A.stats[((size_t)w * A.heads + h) * nq + i] : 0.f;
    }
    __syncthreads();
    const auto [wave, nwaves, c16, g] = att_lane();
    const float *mwin = MK && M.p ? M.p + (size_t)(w % M.win) * nq * nk : nullptr;
    for (int kt = wave; kt < nkt; kt += nwaves) {
        const int j = kt * 16 + c16, jc = min(j, nk - 1);
        const bool jv = j < nk;
        const size_t koff = ((size_t)w * nk + jc) * Ck + h * d, voff = MK ? ((size_t)w * nk + jc) * Cv + h * d : koff;
        float kr[8], vr[8];
        if (ROPE) att_load_row_rot(kr, A.k + koff, cs + jc * (d >> 1), g, d, jv, 1.f);
        else att_load_row(kr, A.k + koff, g, d, jv, 1.f);
        att_load_row(vr, A.v + voff, g, d, jv, 1.f);
        att_f4 dk0 = {0.f, 0.f, 0.f, 0.f}, dk1 = dk0, dv0 = dk0, dv1 = dk0;
        int ix[4], ix1[4];      // (loaded two tiles ahead, unconditionally: as in k_attn_bwd_q)
        if (!ROPE) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ix[r] = A.index[(size_t)min(4 * g + r, nq - 1) * nk + jc];
                ix1[r] = A.index[(size_t)min(16 + 4 * g + r, nq - 1) * nk + jc];
            }
        }
        float mk[4] = {0.f, 0.f, 0.f, 0.f};     // (MK: as in k_attn_bwd_q, the queries 4 g + r of the tile at the lane's key)
        if (MK && mwin) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mk[r] = mwin[(size_t)min(4 * g + r, nq - 1) * nk + jc];
        }
        for (int t = 0; t < nqt; ++t) {
            float b[4];
            int ixn[4];
            float mkn[4] = {0.f, 0.f, 0.f, 0.f};
            if (MK && mwin) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mkn[r] = mwin[(size_t)min(16 * t + 16 + 4 * g + r, nq - 1) * nk + jc];
            }
            if (!ROPE) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    b[r] = att_bias<TLDS>(s_tb, A.table, A.heads, h, ix[r]);
                    ixn[r] = A.index[(size_t)min(16 * t + 32 + 4 * g + r, nq - 1) * nk + jc];
                }
            }
            const float *gq = s_g + (16 * t + 4 * g) * ATT_LD + c16, *qq = s_q + (16 * t + 4 * g) * ATT_LD + c16;
            float g0[4], g1[4], q0[4], q1[4], lse[4], dl[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                g0[r] = gq[r * ATT_LD]; g1[r] = gq[r * ATT_LD + 16];
                q0[r] = qq[r * ATT_LD]; q1[r] = qq[r * ATT_LD + 16];
                lse[r] = s_lse[16 * t + 4 * g + r]; dl[r] = s_delta[16 * t + 4 * g + r];
            }
            const att_f4 sc = att_tile(s_q, 16 * t, c16, g, kr);       // [query 16 t + 4 g + r][key j], the forward's bits
            const att_f4 dp = att_tile(s_g, 16 * t, c16, g, vr);
            float p[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * t + 4 * g + r;
                p[r] = (jv && i < nq) ? att_exp((ROPE ? sc[r] : MK ? (sc[r] + b[r]) + mk[r] : sc[r] + b[r]) - lse[r]) : 0.f;
                ds[r] = p[r] * (dp[r] - dl[r]);
                att_shift(ix[r], ix1[r], ixn[r]);
                if (MK) mk[r] = mkn[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dv0 = att_mfma(p[r], g0[r], dv0);
                dk0 = att_mfma(ds[r], q0[r], dk0);
                dv1 = att_mfma(p[r], g1[r], dv1);
                dk1 = att_mfma(ds[r], q1[r], dk1);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jo = kt * 16 + 4 * g + r;
            float u0 = 0.f, u1 = 0.f;
            if (ROPE) {         // (before the row's test: the shuffle wants the whole wave)
                u0 = att_unrot(dk0[r], cs, min(jo, nk - 1), d >> 1, c16, d);
                u1 = att_unrot(dk1[r], cs, min(jo, nk - 1), d >> 1, c16 + 16, d);
            }
            if (jo < nk) {
                const size_t off = ((size_t)w * nk + jo) * Cgk + h * d, offv = MK ? ((size_t)w * nk + jo) * Cgv + h * d : off;
                if (A.g_k) {
                    if (c16 < d) att_st(A.g_k + off + c16, ROPE ? u0 : dk0[r]);
                    if (c16 + 16 < d) att_st(A.g_k + off + c16 + 16, ROPE ? u1 : dk1[r]);
                }
                if (A.g_v) {
                    if (c16 < d) att_st(A.g_v + offv + c16, dv0[r]);
                    if (c16 + 16 < d) att_st(A.g_v + offv + c16 + 16, dv1[r]);
                }
            }
        }
    }
}

// cossin[h, n, j] = (cos, sin) of angles[h, n, j], once per call: the accurate sincosf (angles reach tens of radians, where the
// hardware's v_sin_f32 / v_cos_f32 lose the bits the scores need), read by every workgroup of the three attention kernels
__global__ __launch_bounds__(256) void k_attn_cossin(AttnAux A)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.heads * A.arows * (A.d >> 1)) return;
    float sn, cs;
    sincosf(A.angles[e], &sn, &cs);
    reinterpret_cast<float2 *>(A.cossin)[e] = make_float2(cs, sn);
}

// d L / d angles[h, n, j] = sum over windows of Im(conj(x) g_x), x = q (n < nq) and x = k (n < nk): the column pair (2 j, 2 j + 1)
// of head h and token n of the UN-rotated input and of its gradient.  One thread per angle; blockIdx.y = a slice of `achunk`
// consecutive windows, added in window order (q's term, then k's) into the slice's partial (or g_angles itself when there is one
// slice).  Rows past both nq and nk get exactly 0.
template <typename T = float>
__global__ __launch_bounds__(256) void k_attn_angle_grad(AttnArgsT<T> A)
{
    const int hd = A.d >> 1, per = A.heads * A.arows * hd;
    const int e = blockIdx.x * 256 + threadIdx.x, slice = blockIdx.y;
    if (e >= per) return;
    const int j = e % hd, n = (e / hd) % A.arows, h = e / (hd * A.arows);
    const int C = A.heads * A.d, col = h * A.d + 2 * j;
    const int w0 = slice * A.achunk, w1 = min(A.windows, w0 + A.achunk);
    float a = 0.f;
    for (int w = w0; w < w1; ++w) {
        if (n < A.nq) {
            const size_t off = ((size_t)w * A.nq + n) * C + col;
            const float2 x = att_ld2(A.q + off), gx = att_ld2(A.g_q + off);
            a = fmaf(x.x, gx.y, a);
            a = fmaf(-x.y, gx.x, a);
        }
        if (n < A.nk) {
            const size_t off = ((size_t)w * A.nk + n) * C + col;
            const float2 x = att_ld2(A.k + off), gx = att_ld2(A.g_k + off);
            a = fmaf(x.x, gx.y, a);
            a = fmaf(-x.y, gx.x, a);
        }
    }
    (A.aslices == 1 ? A.g_angles : A.part + (size_t)slice * per)[e] = a;
}

// g_angles = the slices' partials added in slice order
__global__ __launch_bounds__(256) void k_attn_angle_sum(AttnAux A)
{
    const int per = A.heads * A.arows * (A.d >> 1), e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float a = A.part[e];
    for (int s = 1; s < A.aslices; ++s) a += A.part[(size_t)s * per + e];
    A.g_angles[e] = a;
}

// ---- the host layer: one path for the four descriptor families (the head comment has the plan) ------------------------
constexpr int ATT_ANGLE_CHUNK = 8;      // windows a thread of k_attn_angle_grad adds, at least
constexpr int ATT_ANGLE_SLICES = 64;    // slices (partials per angle), at most

inline int attn_angle_chunk(int windows) { return std::max((windows + ATT_ANGLE_SLICES - 1) / ATT_ANGLE_SLICES, ATT_ANGLE_CHUNK); }
inline int attn_angle_slices(int windows) { return (windows + attn_angle_chunk(windows) - 1) / attn_angle_chunk(windows); }

// true when one of the pointers is not a multiple of `to` (an activation pointer the call does not need may be null)
inline bool attn_misaligned(uintptr_t to, std::initializer_list<const void *> ps)
{
    for (const void *p : ps) if ((uintptr_t)p & (to - 1)) return true;
    return false;
}

// A family states what its descriptor D must hold -- every check returns the message of the first defect, or nullptr, for a
// forward or (`bwd`) a backward -- and fills its own fields of the kernels' arguments.  T: the activations' element type.
// The biased family (gsasr_window_attn, gsasr_window_attn_bf16):
template <typename D, typename ELEM>
struct AttnBiased {
    typedef ELEM T;
    static constexpr bool ROPE = false, MASKED = false;
    typedef AttnArgsT<ELEM> ARGS;
    static constexpr const char *NULL_DESC = "null window-attention descriptor", *TOO_MANY = "windows * heads or table_rows * heads exceeds 2^31 - 1";
    static const char *bad_size(const D *a)
    {
        return a->head_dim < 1 || a->head_dim > ATT_MAX_D ? "need 1 <= head_dim <= 32" : a->table_rows < 1 ? "table_rows must be at least 1" : nullptr;
    }
    static long long side_elems(const D *a) { return (long long)a->table_rows * a->heads; }
    static const char *missing(const D *a, bool bwd)
    {
        const bool fwd = a->q && a->k && a->v && a->table && a->index && a->out;
        if (!bwd) return fwd ? nullptr : "null q, k, v, table, index or out pointer";
        return fwd && a->stats && a->grad_out ? nullptr : "null q, k, v, table, index, out, stats or grad_out pointer";
    }
    static const char *misaligned(const D *a, bool bwd)
    {
        if (sizeof(T) != 2) return nullptr;
        if (!bwd) return attn_misaligned(2, {a->q, a->k, a->v, a->out}) ? "q, k, v and out must be 2-byte aligned" : nullptr;
        return attn_misaligned(2, {a->q, a->k, a->v, a->out, a->grad_out, a->g_q, a->g_k, a->g_v}) ? "q, k, v, out, grad_out, g_q, g_k and g_v must be 2-byte aligned" : nullptr;
    }
    static int wslots(const D *a) { return a->windows < ATT_TAB_WG ? a->windows : ATT_TAB_WG; }
    // d table (k_attn_bwd_q's TAB): 0 none, 1 binned in LDS into partial columns, 2 double atomics on the scratch
    static int tab(const D *a) { return !a->g_table ? 0 : a->table_rows <= ATT_TAB_LDS ? 1 : 2; }
    static const char *bad_scratch(const D *a)
    {
        if (tab(a) && !a->scratch) return "null scratch pointer (the table gradient needs gsasr_window_attn_scratch_bytes)";
        return tab(a) == 2 && ((uintptr_t)a->scratch & 7) ? "scratch must be 8-byte aligned" : nullptr;
    }
    // the backward's partial table columns (one per window slot and head), or above ATT_TAB_LDS rows the table's sums in double
    static size_t scratch(const D *a)
    {
        return align_up((tab(a) == 2 ? sizeof(double) : tab(a) * wslots(a) * sizeof(float)) * a->heads * a->table_rows, 256);
    }
    static void fill(AttnArgsT<T> &A, const D *a)
    {
        A.table = a->table; A.index = a->index; A.g_table = a->g_table; A.rows = a->table_rows; A.wslots = wslots(a);
        A.vec = a->nk % 4 == 0 && ((uintptr_t)a->index & 15) == 0;
    }
};

// the rotary family (gsasr_window_attn_rope, gsasr_window_attn_rope_bf16): no table, no index; the angles and their (cos, sin)
template <typename D, typename ELEM>
struct AttnRotary {
    typedef ELEM T;
    static constexpr bool ROPE = true, MASKED = false;
    typedef AttnArgsT<ELEM> ARGS;
    static constexpr const char *NULL_DESC = "null rotary window-attention descriptor", *TOO_MANY = "windows * heads or heads * angle_rows * head_dim / 2 exceeds 2^31 - 1";
    static const char *bad_size(const D *a)
    {
        if (a->head_dim < 2 || a->head_dim > ATT_MAX_D || a->head_dim % 2) return "need an even head_dim, 2 <= head_dim <= 32";
        return a->angle_rows < (a->nq > a->nk ? a->nq : a->nk) ? "angle_rows must be at least max(nq, nk)" : nullptr;
    }
    static long long side_elems(const D *a) { return (long long)a->angle_rows * a->heads * (a->head_dim / 2); }
    static const char *missing(const D *a, bool bwd)
    {
        const bool both = a->q && a->k && a->v && a->out && a->cossin;
        if (!bwd) return both && a->angles ? nullptr : "null q, k, v, angles, out or cossin pointer";
        if (!both || !a->stats || !a->grad_out) return "null q, k, v, out, stats, grad_out or cossin pointer";
        return a->g_angles && (!a->g_q || !a->g_k) ? "g_angles needs g_q and g_k (it is formed from them)" : nullptr;
    }
    static const char *misaligned(const D *a, bool bwd)
    {
        const bool cs = attn_misaligned(8, {a->cossin});
        if (sizeof(T) != 2) {       // (column pairs are read and written 8 bytes at a time)
            if (!bwd) return cs || attn_misaligned(8, {a->q, a->k}) ? "q, k and cossin must be 8-byte aligned" : nullptr;
            return cs || attn_misaligned(8, {a->q, a->k, a->g_q, a->g_k}) ? "q, k, cossin, g_q and g_k must be 8-byte aligned" : nullptr;
        }
        if (!bwd) return cs || attn_misaligned(4, {a->q, a->k, a->v, a->out}) ? "q, k, v and out must be 4-byte aligned and cossin 8-byte aligned" : nullptr;
        return cs || attn_misaligned(4, {a->q, a->k, a->v, a->out, a->grad_out, a->g_q, a->g_k, a->g_v})
                   ? "q, k, v, out, grad_out, g_q, g_k and g_v must be 4-byte aligned and cossin 8-byte aligned" : nullptr;
    }
    static int tab(const D *) { return 0; }
    // the slices' partial angle gradients of the backward
    static size_t scratch(const D *a)
    {
        const int slices = attn_angle_slices(a->windows);
        return a->g_angles && slices > 1 ? align_up((size_t)slices * a->heads * a->angle_rows * (a->head_dim / 2) * sizeof(float), 256) : 0;
    }
    static const char *bad_scratch(const D *a)
    {
        return scratch(a) && !a->scratch ? "null scratch pointer (the angle gradient needs gsasr_window_attn_rope_scratch_bytes)" : nullptr;
    }
    static void fill(AttnArgsT<T> &A, const D *a)
    {
        A.wslots = a->windows;      // (no table to bin: one workgroup of k_attn_bwd_q per window and head)
        A.angles = a->angles; A.cossin = a->cossin; A.g_angles = a->g_angles; A.arows = a->angle_rows;
        A.achunk = attn_angle_chunk(a->windows); A.aslices = attn_angle_slices(a->windows);
    }
};

// the masked family (gsasr_window_attn_masked, gsasr_window_attn_masked_bf16): the biased family's rules and fields, a mask
// per window modulo mask_windows and a row pitch for each of q, k, v, g_q, g_k, g_v (0: heads * head_dim)
template <typename D, typename ELEM>
struct AttnMasked : AttnBiased<D, ELEM> {
    typedef AttnBiased<D, ELEM> B;
    typedef ELEM T;
    static constexpr bool MASKED = true;
    typedef AttnArgsMT<ELEM> ARGS;
    static const char *bad_size(const D *a)
    {
        if (const char *msg = B::bad_size(a)) return msg;
        if (a->mask_windows < 0) return "mask_windows must not be negative";
        if (a->mask_windows && a->windows % a->mask_windows) return "windows must be a multiple of mask_windows";
        const long long c = (long long)a->heads * a->head_dim;
        for (long long p : {a->pitch_q, a->pitch_k, a->pitch_v, a->pitch_gq, a->pitch_gk, a->pitch_gv})
            if (p && p < c) return "a non-zero pitch must be at least heads * head_dim";
        return nullptr;
    }
    static const char *missing(const D *a, bool bwd)
    {
        if (const char *msg = B::missing(a, bwd)) return msg;
        return (a->mask != nullptr) != (a->mask_windows != 0) ? "mask and mask_windows must be set together (NULL and 0: no mask)" : nullptr;
    }
    static void fill(AttnArgsMT<T> &A, const D *a)
    {
        B::fill(A, a);
        const long long c = (long long)a->heads * a->head_dim;
        auto pitch = [c](long long p) { return p ? p : c; };
        A.mask = a->mask; A.mwin = a->mask_windows > 0 ? a->mask_windows : 1;
        A.mvec = a->nk % 4 == 0 && ((uintptr_t)a->mask & 15) == 0;
        A.pq = pitch(a->pitch_q); A.pk = pitch(a->pitch_k); A.pv = pitch(a->pitch_v);
        A.pgq = pitch(a->pitch_gq); A.pgk = pitch(a->pitch_gk); A.pgv = pitch(a->pitch_gv);
        // the bf16 forward's load width: every row of q, k, v must keep the alignment of the first (attn_args has the bases)
        if (sizeof(T) == 2 && A.ldvec > 1 && ((A.pq | A.pk | A.pv) & (A.ldvec - 1))) A.ldvec = (A.pq | A.pk | A.pv) & 1 ? 1 : 2;
    }
};

template <typename D> struct AttnFamily;
template <> struct AttnFamily<gsasr_window_attn_masked> : AttnMasked<gsasr_window_attn_masked, float> {};
template <> struct AttnFamily<gsasr_window_attn_masked_bf16> : AttnMasked<gsasr_window_attn_masked_bf16, att_bf> {};
template <> struct AttnFamily<gsasr_window_attn> : AttnBiased<gsasr_window_attn, float> {};
template <> struct AttnFamily<gsasr_window_attn_bf16> : AttnBiased<gsasr_window_attn_bf16, att_bf> {};
template <> struct AttnFamily<gsasr_window_attn_rope> : AttnRotary<gsasr_window_attn_rope, float> {};
template <> struct AttnFamily<gsasr_window_attn_rope_bf16> : AttnRotary<gsasr_window_attn_rope_bf16, att_bf> {};

// the sizes, flags and scale of a descriptor (no pointer is looked at), then with `call` = 1 a forward's or 2 a backward's pointers
template <typename D>
int attn_check(const D *a, int call = 0)
{
    typedef AttnFamily<D> F;
    if (!a) return fail(GSASR_ERR_ARG, F::NULL_DESC);
    if (a->windows < 1 || a->heads < 1) return fail(GSASR_ERR_ARG, "windows and heads must be at least 1");
    if (a->nq < 1 || a->nq > ATT_MAX_N || a->nk < 1 || a->nk > ATT_MAX_N) return fail(GSASR_ERR_ARG, "need 1 <= nq, nk <= 256");
    if (const char *msg = F::bad_size(a)) return fail(GSASR_ERR_ARG, msg);
    if (a->flags) return fail(GSASR_ERR_ARG, "unknown flags (none are defined)");
    if (!(a->scale == a->scale)) return fail(GSASR_ERR_ARG, "scale is NaN");
    if ((long long)a->windows * a->heads > 0x7fffffffLL || F::side_elems(a) > 0x7fffffffLL) return fail(GSASR_ERR_ARG, F::TOO_MANY);
    const char *msg = call ? F::missing(a, call == 2) : nullptr;
    if (call && !msg) msg = F::misaligned(a, call == 2);
    if (call == 2 && !msg) msg = F::bad_scratch(a);
    return msg ? fail(GSASR_ERR_ARG, msg) : GSASR_OK;
}

// never 0 for a valid descriptor
template <typename D>
size_t attn_scratch_bytes(const D *a) { return attn_check(a) ? 0 : 256 + AttnFamily<D>::scratch(a); }

template <typename D>
typename AttnFamily<D>::ARGS attn_args(const D *a)
{
    typename AttnFamily<D>::ARGS A = {};
    A.q = a->q; A.k = a->k; A.v = a->v; A.out = a->out; A.o = a->out; A.stats = a->stats;
    A.grad_out = a->grad_out; A.g_q = a->g_q; A.g_k = a->g_k; A.g_v = a->g_v; A.part = (float *)a->scratch;
    A.windows = a->windows; A.heads = a->heads; A.nq = a->nq; A.nk = a->nk; A.d = a->head_dim; A.scale = a->scale;
    // elements per global load of the bf16 forward: by the alignment of a head's slice (its offset is 2 h d bytes into a row of 2 H d)
    const uintptr_t any = (uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v;
    A.ldvec = A.d % 8 == 0 && (any & 15) == 0 ? 8 : A.d % 2 == 0 && (any & 3) == 0 ? 2 : 1;
    AttnFamily<D>::fill(A, a);
    return A;
}

template <typename T>
AttnAux attn_aux(const AttnArgsT<T> &A) { return {A.g_table, A.part, A.heads, A.angles, A.cossin, A.d, A.g_angles, A.arows, A.rows, A.wslots, A.aslices}; }

// waves per workgroup, one 16-row tile per wave and turn: three when that deals the tiles evenly and four do not (144 tokens = 9 tiles)
inline int attn_waves(int n)
{
    const int tiles = (n + 15) / 16;
    return tiles % 4 != 0 && tiles % 3 == 0 ? 3 : 4;
}

template <typename K, typename ARGS>
int attn_launch(K kernel, dim3 grid, int waves, size_t lds, hipStream_t st, const ARGS &A)
{
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(64 * waves), lds, st, A);
    HIP_TRY(hipGetLastError());
    return GSASR_OK;
}

// f(std::integral_constant<int, N>) for the first N of the list with v <= N (the last one otherwise): a runtime value as a
// template argument.  Every MAXT, STATS, TLDS and TAB of a launch comes through here
template <int N, int... MORE, typename F>
int att_pick(int v, F &&f)
{
    if constexpr (sizeof...(MORE) == 0) return f(std::integral_constant<int, N>());
    else return v <= N ? f(std::integral_constant<int, N>()) : att_pick<MORE...>(v, f);
}

template <typename D>
int attn_forward(const D *a, void *stream)
{
    typedef AttnFamily<D> F;
    typedef typename F::T T;
    if (int rc = attn_check(a, 1)) return rc;
    const typename F::ARGS A = attn_args(a);
    hipStream_t st = (hipStream_t)stream;
    if (F::ROPE) if (int rc = attn_launch(k_attn_cossin, (unsigned)((A.heads * A.arows * (A.d / 2) + 255) / 256), 4, 0, st, attn_aux(A))) return rc;
    const unsigned grid = (unsigned)(A.windows * A.heads);
    const int waves = attn_waves(A.nq);
    const bool tlds = !F::ROPE && A.rows <= ATT_TAB_LDS;
    // MAXT by the key tiles.  The masked family has one for exactly four: SwinIR's 64 keys, where it is a third shorter than MAXT 9
    // (DESIGN.md 3.2i); the other families' shipped shapes have 9 and 16 tiles and keep their three
    auto launch = [&](auto maxt) {
        return att_pick<0, 1>(A.stats != nullptr, [&](auto stats) { return att_pick<0, 1>(tlds, [&](auto tl) {
        constexpr int MAXT = decltype(maxt)::value;
        constexpr bool STATS = decltype(stats)::value, TLDS = decltype(tl)::value && !F::ROPE;
        if constexpr (sizeof(T) == 2) return attn_launch(k_attn_fwd_bf<MAXT, STATS, TLDS, F::ROPE, F::MASKED>, grid, waves, AttLdsFwdBf(A.nk, TLDS ? A.rows : 0).bytes(), st, A);
        else return attn_launch(k_attn_fwd<MAXT, STATS, TLDS, F::ROPE, F::MASKED>, grid, waves, AttLdsQ(A.nk, TLDS ? A.rows : 0).bytes(), st, A);
    }); }); };
    if constexpr (F::MASKED) return att_pick<3, 4, 9, 16>((A.nk + 15) / 16, launch);
    else return att_pick<3, 9, 16>((A.nk + 15) / 16, launch);
}

// d table after k_attn_bwd_q: the partial columns added in a fixed order (TAB 1), or the double sums rounded (TAB 2)
template <typename T>
int attn_table_tail(const AttnArgsT<T> &A, int tab, hipStream_t st)
{
    const unsigned n = (unsigned)(A.rows * A.heads);
    return tab == 1 ? attn_launch(k_attn_table_sum, (n + 31) / 32, 4, 0, st, attn_aux(A)) : attn_launch(k_attn_table_round, (n + 255) / 256, 4, 0, st, attn_aux(A));
}

// d angles after both kernels: from q, k and their gradients, a slice of windows per thread, then the slices in order
template <typename T>
int attn_angle_tail(const AttnArgsT<T> &A, hipStream_t st)
{
    if (!A.g_angles) return GSASR_OK;
    const unsigned blocks = (unsigned)((A.heads * A.arows * (A.d / 2) + 255) / 256);
    if (int rc = attn_launch(k_attn_angle_grad<T>, dim3(blocks, (unsigned)A.aslices), 4, 0, st, A)) return rc;
    return A.aslices > 1 ? attn_launch(k_attn_angle_sum, blocks, 4, 0, st, attn_aux(A)) : GSASR_OK;
}

// the backward of every family: k_attn_bwd_q (dq, d table), k_attn_bwd_kv (dk, dv), each followed by the family's own tail
template <typename D>
int attn_backward(const D *a, void *stream)
{
    typedef AttnFamily<D> F;
    typedef typename F::T T;
    if (int rc = attn_check(a, 2)) return rc;
    const typename F::ARGS A = attn_args(a);
    hipStream_t st = (hipStream_t)stream;
    const int tab = F::tab(a);
    const bool tlds = !F::ROPE && A.rows <= ATT_TAB_LDS;
    if (A.g_q || tab) {
        if (tab == 2) HIP_TRY(hipMemsetAsync(A.part, 0, (size_t)A.rows * A.heads * sizeof(double), st));
        const size_t lds = AttLdsQ(A.nk, tlds ? A.rows : 0, tab == 1 ? A.rows : 0).bytes();
        int rc = att_pick<0, 1, 2>(tab, [&](auto t) { return att_pick<0, 1>(tlds, [&](auto tl) {
            constexpr int TAB = F::ROPE ? 0 : decltype(t)::value;
            constexpr bool TLDS = TAB == 1 || (TAB == 0 && !F::ROPE && decltype(tl)::value);     // (TAB 1 is the table in LDS, TAB 2 is not)
            return attn_launch(k_attn_bwd_q<TAB, TLDS, F::ROPE, T, F::MASKED>, (unsigned)(A.wslots * A.heads), attn_waves(A.nq), lds, st, A);
        }); });
        if (!rc && tab) rc = attn_table_tail(A, tab, st);
        if (rc) return rc;
    }
    if (A.g_k || A.g_v) {
        const size_t lds = AttLdsKV(A.nq, tlds ? A.rows : 0).bytes();
        if (int rc = att_pick<0, 1>(tlds, [&](auto tl) {
                constexpr bool TLDS = decltype(tl)::value && !F::ROPE;
                return attn_launch(k_attn_bwd_kv<TLDS, F::ROPE, T, F::MASKED>, (unsigned)(A.windows * A.heads), attn_waves(A.nk), lds, st, A);
            })) return rc;
    }
    return F::ROPE ? attn_angle_tail(A, st) : GSASR_OK;
}

}  // namespace

extern "C" {

size_t gsasr_window_attn_scratch_bytes(const gsasr_window_attn *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_forward(const gsasr_window_attn *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_backward(const gsasr_window_attn *a, void *stream) { return attn_backward(a, stream); }

size_t gsasr_window_attn_rope_scratch_bytes(const gsasr_window_attn_rope *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_rope_forward(const gsasr_window_attn_rope *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_rope_backward(const gsasr_window_attn_rope *a, void *stream) { return attn_backward(a, stream); }

// bf16 activations: the forward on the bf16 matrix instruction, the backward the fp32 kernels on att_bf
size_t gsasr_window_attn_bf16_scratch_bytes(const gsasr_window_attn_bf16 *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_bf16_forward(const gsasr_window_attn_bf16 *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_bf16_backward(const gsasr_window_attn_bf16 *a, void *stream) { return attn_backward(a, stream); }

// the masked family: a mask per window (modulo mask_windows) after the bias, q, k, v and their gradients at their own row pitches
size_t gsasr_window_attn_masked_scratch_bytes(const gsasr_window_attn_masked *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_masked_forward(const gsasr_window_attn_masked *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_masked_backward(const gsasr_window_attn_masked *a, void *stream) { return attn_backward(a, stream); }

size_t gsasr_window_attn_masked_bf16_scratch_bytes(const gsasr_window_attn_masked_bf16 *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_masked_bf16_forward(const gsasr_window_attn_masked_bf16 *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_masked_bf16_backward(const gsasr_window_attn_masked_bf16 *a, void *stream) { return attn_backward(a, stream); }

size_t gsasr_window_attn_rope_bf16_scratch_bytes(const gsasr_window_attn_rope_bf16 *a) { return attn_scratch_bytes(a); }
int gsasr_window_attn_rope_bf16_forward(const gsasr_window_attn_rope_bf16 *a, void *stream) { return attn_forward(a, stream); }
int gsasr_window_attn_rope_bf16_backward(const gsasr_window_attn_rope_bf16 *a, void *stream) { return attn_backward(a, stream); }

}  // extern "C"
