// The per-row system of iALS (include/recad_hip.h): staging of a row's entries in LDS, A_u on the fp32 MFMA, b_u, the Cholesky
// factorisation and the triangular solves inside LDS.  Shared by ials.hip (rk_ials_half_sweep, rk_ials_system, rk_ials_gram) and
// pga.hip (rk_ials_solve_rhs), which instantiate the same device code: what one factorises the other factorises to the bit.
#pragma once
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "common.h"

typedef float ia_f32x4 __attribute__((ext_vector_type(4)));

static constexpr int kIaThreads = 256;
static constexpr int kIaChunk = RK_IALS_CHUNK;                   // entries (rows of Y) staged at once
static constexpr int kIaGramRows = RK_IALS_GRAM_ROWS;            // rows of Y in one Gram partial
static_assert(kIaChunk == 64 && kIaGramRows % kIaChunk == 0, "the staging thread map; a Gram block is whole chunks");
static_assert(RK_IALS_MAX_DIM == 128, "two elements per lane in the triangular solves, eight tiles a side");

__host__ __device__ inline int ia_dp(int d) { return (d + 15) & ~15; }
// Row stride of the staged entries: 16 or 48 mod 64, so the four rows an MFMA operand reads (16 lanes each) fall into four
// different quarters of the 64 banks.
__host__ __device__ inline int ia_ldy(int dp) { return dp | 16; }
// Odd row stride of A_u: a column walk (the Cholesky scale, the forward substitution) is conflict-free.
__host__ __device__ inline int ia_lda(int dp) { return dp + 1; }

// LDS layout in floats: [A: dp * lda (with_a), and in the same place Y: chunk * ldy] [w: chunk] [c: chunk] [col: chunk] [b: dp].
// A_u is written only after the last staged chunk has been consumed, so the two share their storage: 21 KiB a row at d = 64.
struct IaLds {
    float *A, *Y, *w, *c, *b;
    int *col;
};
__host__ __device__ inline size_t ia_lds_shared(int dp, bool with_a)
{
    const size_t a = with_a ? (size_t)dp * ia_lda(dp) : 0, y = (size_t)kIaChunk * ia_ldy(dp);
    return a > y ? a : y;
}
__host__ __device__ inline size_t ia_lds_floats(int dp, bool with_a) { return ia_lds_shared(dp, with_a) + 3 * kIaChunk + dp; }
__device__ __forceinline__ IaLds ia_carve(float *base, int dp, bool with_a)
{
    IaLds l;
    l.A = base;
    l.Y = base;
    l.w = base + ia_lds_shared(dp, with_a);
    l.c = l.w + kIaChunk;
    l.col = reinterpret_cast<int *>(l.c + kIaChunk);
    l.b = l.c + 2 * kIaChunk;
    return l;
}

// The lower-triangle tiles of an NT x NT tile grid in row-major order; wave w owns tiles w, w + 4, ...: S accumulators.
template <int NT>
struct IaTiles {
    static constexpr int T = NT * (NT + 1) / 2, S = (T + 3) / 4;
};
template <int NT>
struct IaAcc {
    ia_f32x4 acc[IaTiles<NT>::S];
    int ro[IaTiles<NT>::S], co[IaTiles<NT>::S];                   // first row and column of the tile; ro < 0: no tile

    __device__ __forceinline__ void init(int wave)
    {
#pragma unroll
        for (int s = 0; s < IaTiles<NT>::S; ++s) {
            const int t = wave + 4 * s;
            int I = 0;
            while ((I + 1) * (I + 2) / 2 <= t) ++I;
            const bool have = t < IaTiles<NT>::T;
            ro[s] = have ? 16 * I : -1;
            co[s] = have ? 16 * (t - I * (I + 1) / 2) : 0;
            acc[s] = ia_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    // acc += sum over the staged rows [0, rows4) of (w y)(y)^T on my tiles: the A operand is scaled on load, one rounding.
    // Lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15].
    __device__ __forceinline__ void add_rows(const IaLds &l, int ldy, int rows4, int lane)
    {
        const int lr = lane & 15, lk = lane >> 4;
#pragma unroll 1
        for (int k0 = 0; k0 < rows4; k0 += 4) {
            const float *row = l.Y + (k0 + lk) * ldy + lr;
            const float w = l.w[k0 + lk];
#pragma unroll
            for (int s = 0; s < IaTiles<NT>::S; ++s)
                if (ro[s] >= 0) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(w * row[ro[s]], row[co[s]], acc[s], 0, 0, 0);
        }
    }
};

// s + fl(c * y): two roundings, never one fused multiply-add
__device__ __forceinline__ float ia_add_term(float s, float c, float y)
{
#pragma clang fp contract(off)
    const float term = c * y;
    return s + term;
}

// Stages rows [0, rows4) of the chunk: row e is Y[ids[e]] (ids < 0: zeros), columns [d, dp) zero.  l.col holds the ids.
__device__ __forceinline__ void ia_stage_rows(const IaLds &l, int d, int dp, int ldy, int rows4, const float *__restrict__ Y)
{
    for (int at = threadIdx.x; at < rows4 * dp; at += kIaThreads) {
        const int e = at / dp, k = at - e * dp;
        const int c = l.col[e];
        l.Y[e * ldy + k] = (c >= 0 && k < d) ? Y[(size_t)c * d + k] : 0.0f;
    }
}

// The system of the row whose entries are [beg, end): A_u into l.A (the lower triangle, and what the diagonal tiles hold above
// it, which nothing reads), b_u into l.b.  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void ia_build_system(const IaLds &l, int n_cols, int d, const float *__restrict__ G, const int *__restrict__ col,
                                                const float *__restrict__ val, int beg, int end, float alpha, const float *__restrict__ Y)
{
    constexpr int dp = 16 * NT;
    const int ldy = ia_ldy(dp), lda = ia_lda(dp);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    IaAcc<NT> t;
    t.init(wave);
    float bk = 0.0f;                                               // component tid of b_u
#pragma unroll 1
    for (int e0 = beg; e0 < end; e0 += kIaChunk) {
        const int cnt = min(kIaChunk, end - e0), rows4 = (cnt + 3) & ~3;
        __syncthreads();                                           // the chunk before this one has been consumed
        if (tid < kIaChunk) {
#pragma clang fp contract(off)
            int c = -1;
            float w = 0.0f, cc = 0.0f;
            if (tid < cnt) {
                const int ci = col[e0 + tid];
                if ((unsigned)ci < (unsigned)n_cols) {
                    c = ci;
                    w = alpha * (float)(int)val[e0 + tid];
                    cc = 1.0f + w;
                }
            }
            l.col[tid] = c;
            l.w[tid] = w;
            l.c[tid] = cc;
        }
        __syncthreads();
        ia_stage_rows(l, d, dp, ldy, rows4, Y);
        __syncthreads();
        t.add_rows(l, ldy, rows4, lane);
        if (tid < d)
            for (int e = 0; e < cnt; ++e) bk = ia_add_term(bk, l.c[e], l.Y[e * ldy + tid]);
    }
    __syncthreads();                                               // the last chunk has been consumed: A_u takes its place
    // C/D map of the 16 x 16 tile: column lane & 15, row 4 (lane >> 4) + r
#pragma unroll
    for (int s = 0; s < IaTiles<NT>::S; ++s) {
        if (t.ro[s] < 0) continue;
        const int j = t.co[s] + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = t.ro[s] + 4 * (lane >> 4) + r;
            l.A[i * lda + j] = (i < d && j < d) ? G[i * d + j] + t.acc[s][r] : (i == j ? 1.0f : 0.0f);
        }
    }
    if (tid < dp) l.b[tid] = tid < d ? bk : 0.0f;
    __syncthreads();
}

// A = L L^T in place over the lower triangle, right-looking, a column at a time; every operation rounded on its own.  False (in
// every thread) at a pivot that is not a finite number > 0.
__device__ __forceinline__ bool ia_cholesky(int d, int lda, float *A)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
#pragma unroll 1
    for (int p = 0; p < d; ++p) {
        const float piv = A[p * lda + p];                          // the same value in every thread
        if (!(piv > 0.0f) || !isfinite(piv)) return false;
        const float r = sqrtf(piv);
        for (int i = p + 1 + tid; i < d; i += kIaThreads) A[i * lda + p] = A[i * lda + p] / r;
        __syncthreads();                                           // column p is scaled, and everyone holds the pivot
        if (tid == 0) A[p * lda + p] = r;                          // nothing below reads the diagonal of column p
        for (int i = p + 1 + ty; i < d; i += kIaThreads / 32) {
            const float lip = A[i * lda + p];
            for (int j = p + 1 + tx; j <= i; j += 32) {
                const float prod = lip * A[j * lda + p];
                A[i * lda + j] = A[i * lda + j] - prod;
            }
        }
        __syncthreads();
    }
    return true;
}

// x = L^-T L^-1 b by the first wave: lane k holds components k and k + 64 in registers, L is only read.  Column-oriented:
// z_p = b_p / l_pp, b_i <- b_i - fl(l_ip z_p) for i > p; then x_p = z_p / l_pp, z_i <- z_i - fl(l_pi x_p) for i < p.
__device__ __forceinline__ void ia_solve(int d, int lda, const float *A, const float *b, float *__restrict__ x)
{
#pragma clang fp contract(off)
    if (threadIdx.x >= 64) return;
    const int k0 = threadIdx.x, k1 = k0 + 64;
    float v0 = k0 < d ? b[k0] : 0.0f, v1 = k1 < d ? b[k1] : 0.0f;
#pragma unroll 1
    for (int p = 0; p < d; ++p) {
        const float z = __shfl(p < 64 ? v0 : v1, p & 63, 64) / A[p * lda + p];
        if (k0 == p) v0 = z;
        if (k1 == p) v1 = z;
        if (k0 > p && k0 < d) {
            const float prod = A[k0 * lda + p] * z;
            v0 = v0 - prod;
        }
        if (k1 > p && k1 < d) {
            const float prod = A[k1 * lda + p] * z;
            v1 = v1 - prod;
        }
    }
#pragma unroll 1
    for (int p = d - 1; p >= 0; --p) {
        const float xp = __shfl(p < 64 ? v0 : v1, p & 63, 64) / A[p * lda + p];
        if (k0 == p) v0 = xp;
        if (k1 == p) v1 = xp;
        if (k0 < p) {
            const float prod = A[p * lda + k0] * xp;
            v0 = v0 - prod;
        }
        if (k1 < p) {
            const float prod = A[p * lda + k1] * xp;
            v1 = v1 - prod;
        }
    }
    if (k0 < d) x[k0] = v0;
    if (k1 < d) x[k1] = v1;
}

static inline bool ia_bad_dim(int d) { return d < 1 || d > RK_IALS_MAX_DIM; }
static inline bool ia_bad_alpha(float a) { return !isfinite(a) || !(a >= 0.0f); }
static inline bool ia_bad_lambda(float l) { return !isfinite(l) || !(l > 0.0f); }

#define IA_DISPATCH(nt, CALL)       \
    switch (nt) {                   \
    case 1: CALL(1); break;         \
    case 2: CALL(2); break;         \
    case 3: CALL(3); break;         \
    case 4: CALL(4); break;         \
    case 5: CALL(5); break;         \
    case 6: CALL(6); break;         \
    case 7: CALL(7); break;         \
    default: CALL(8); break;        \
    }
