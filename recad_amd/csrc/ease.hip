// EASE victim (Steck 2019): the closed-form item-item model B = I - P diag(1 / diag P), P = (X^T X + lambda I)^-1, from the U x I
// rating CSR and its transpose (rk_pca_transpose).  include/recad_hip.h states the definition.  rk_ease_gram forms A = X^T X +
// lambda I one row per workgroup with integer LDS adds (exact in any arrival order).  rk_ease_invert is a blocked Gauss-Jordan
// sweep without pivoting, in place: per block step one workgroup inverts the pivot block in LDS, a panel kernel forms the
// block-row D A_kj and the block-column -A_ik D (keeping a copy of A_ik in the workspace), and the trailing kernel subtracts
// A_ik (D A_kj), summed on the exact fp32 MFMA, from every other 64 x 64 tile.  Nothing in it adds floats atomically: a tile has one
// owner and its sums run in k order, so two runs give the same bits.  rk_ease_weights turns P into B, rk_ease_scores and
// rk_ease_pair_scores sum q * B[i, j] over a user's entries in column order.
#include <algorithm>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "item_list.h"   // kIkSearchFrom: the gram kernel walks as the neighbour kernels do

typedef float ea_f32x16 __attribute__((ext_vector_type(16)));

static constexpr int kEaThreads = 256;
static constexpr int kEaTile = 64;                              // edge of a panel / trailing tile: four waves, 32 x 32 each
static constexpr int kEaLd = kEaTile + 1;                       // odd leading dimension: rows and columns of a tile are conflict-free
static constexpr int kEaGramBand = 8192;                        // int32 accumulators of one gram workgroup (32 KiB)
static_assert(RK_EASE_BLOCK_LARGE == kEaTile && RK_EASE_BLOCK_SMALL == 32, "a pivot block is at most one tile wide");
static_assert((long long)RK_EASE_MAX_ITEMS / kEaTile <= 65535, "the trailing grid's y dimension");

// ---- gram
// status[1] <- the lowest item whose d_ii reaches 2^24; one wave per item
__global__ __launch_bounds__(256) void ease_diag_check_kernel(int n_items, const int *__restrict__ colptr, const float *__restrict__ cval,
                                                              int *__restrict__ status)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n_items) return;
    long long d = 0;
    for (int e = colptr[i] + lane; e < colptr[i + 1]; e += 64) {
        const long long q = (int)cval[e];
        d += q * q;
    }
    d = wave_sum(d);
    if (lane == 0 && d >= (1LL << 24)) atomicMin(status + 1, i);
}

// One workgroup per item i: row i of A, a band of columns at a time (itemknn_neighbors_kernel's accumulation).
__global__ __launch_bounds__(kEaThreads) void ease_gram_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                               const int *__restrict__ col, const float *__restrict__ val,
                                                               const int *__restrict__ colptr, const int *__restrict__ crow,
                                                               const float *__restrict__ cval, float lambda, float *__restrict__ A)
{
    __shared__ int acc[kEaGramBand];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x;
    const int beg = colptr[i], end = colptr[i + 1];
#pragma unroll 1
    for (int lo = 0; lo < n_items; lo += kEaGramBand) {
        const int bn = min(kEaGramBand, n_items - lo);
        for (int j = tid; j < bn; j += kEaThreads) acc[j] = 0;
        __syncthreads();
        const bool whole = lo == 0 && bn == n_items;
        for (int e = beg + wave; e < end; e += kEaThreads / 64) {
            const int u = crow[e];
            if (u < 0 || u >= n_users) continue;
            const int q = (int)cval[e];
            int s0 = rowptr[u], s1 = rowptr[u + 1];
            if (!whole && s1 - s0 > kIkSearchFrom) {
                s0 = rk_lower_bound(col, s0, s1, lo);
                s1 = rk_lower_bound(col, s0, s1, lo + bn);
            }
            for (int p = s0 + lane; p < s1; p += 64) {
                const int j = col[p] - lo;
                if ((unsigned)j < (unsigned)bn) atomicAdd(acc + j, q * (int)val[p]);
            }
        }
        __syncthreads();
        for (int j = tid; j < bn; j += kEaThreads) {
            float a = (float)acc[j];
            if (lo + j == i) a = a + lambda;
            A[(size_t)i * n_items + lo + j] = a;
        }
        __syncthreads();
    }
}

RK_EXPORT int rk_ease_gram(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                           const int32_t *colptr, const int32_t *crow, const float *cval, float lambda, float *A, int32_t *status,
                           void *stream)
{
    if (n_users <= 0 || !rowptr || !col || !val || !colptr || !crow || !cval || !A || !status) RK_FAIL(RK_EINVAL, "rk_ease_gram: bad arguments");
    if (n_items < 1 || n_items > RK_EASE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_ease_gram: %d items outside 1..%d", n_items, RK_EASE_MAX_ITEMS);
    if (!isfinite(lambda) || !(lambda > 0.0f)) RK_FAIL(RK_EINVAL, "rk_ease_gram: lambda = %g is not a finite positive number", (double)lambda);
    hipStream_t s = (hipStream_t)stream;
    int st[2] = {0, INT_MAX};
    RK_HIP(rk_set_status(status, 0, INT_MAX, s));
    hipLaunchKernelGGL(ease_diag_check_kernel, dim3((n_items + 3) / 4), dim3(256), 0, s, n_items, colptr, cval, status);
    RK_CHECK_LAUNCH();
    RK_HIP(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    const bool bad = st[1] != INT_MAX;
    RK_HIP(rk_set_status(status, bad ? RK_EASE_BAD_GRAM : 0, bad ? st[1] : -1, s));
    if (bad) RK_FAIL(RK_EINVAL, "rk_ease_gram: item %d has a squared norm of 2^24 or more", st[1]);
    hipLaunchKernelGGL(ease_gram_kernel, dim3(n_items), dim3(kEaThreads), 0, s, n_users, n_items, rowptr, col, val, colptr, crow, cval,
                       lambda, A);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- invert
// Inverts A[k0 .. k0 + bk)^2 in LDS by an unblocked Gauss-Jordan sweep, one workgroup.  Thread (r0, c) owns the elements (r0 + 4 q, c):
// per pivot it reads the pivot row and column, then (after a barrier) writes its own elements only.  The padding beyond bk is the
// identity, which the sweep leaves alone.  A pivot that is not a finite number > 0 ends the sweep: status = {RK_EASE_NOT_SPD, index}.
__global__ __launch_bounds__(kEaThreads) void ease_pivot_kernel(int n, float *__restrict__ A, int k0, int bk, int *__restrict__ status)
{
    __shared__ float S[kEaTile][kEaLd];
    if (status[0] != 0) return;
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int r = r0; r < kEaTile; r += 4)
        S[r][c] = (r < bk && c < bk) ? A[(size_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0f : 0.0f);
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < bk; ++p) {
        const float piv = S[p][p];
        if (!(piv > 0.0f) || !isfinite(piv)) {                         // the same value in every thread
            if (threadIdx.x == 0) {
                status[1] = k0 + p;
                status[0] = RK_EASE_NOT_SPD;
            }
            return;
        }
        const float inv = 1.0f / piv;
        float f[kEaTile / 4];
#pragma unroll
        for (int q = 0; q < kEaTile / 4; ++q) f[q] = S[r0 + 4 * q][p];
        const float rs = c == p ? inv : S[p][c] * inv;                // the new pivot row at my column
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kEaTile / 4; ++q) {
            const int r = r0 + 4 * q;
            S[r][c] = r == p ? rs : (c == p ? -f[q] * inv : S[r][c] - f[q] * rs);
        }
        __syncthreads();
    }
    for (int r = r0; r < bk; r += 4)
        if (c < bk) A[(size_t)(k0 + r) * n + k0 + c] = S[r][c];
}

// acc += X Y over k in [0, kn) for the wave's 32 x 32 quarter (wr, wc) of a 64 x 64 tile; sX[i][k], sY[j][k].  Register r of the
// accumulator is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31 (csrc/gemm.h).
__device__ __forceinline__ ea_f32x16 ea_tile_mma(const float (*sX)[kEaLd], const float (*sY)[kEaLd], int wr, int wc, int lane, int kn,
                                                 ea_f32x16 acc)
{
    const int lr = lane & 31, lk = lane >> 5;
    for (int kk = 0; kk < kn; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sX[wr * 32 + lr][kk + lk], sY[wc * 32 + lr][kk + lk], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ int ea_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// Workgroups [0, nT): 64 columns of the block-row, A[K, j] <- D A[K, j] for j outside K.  Workgroups [nT, 2 nT): 64 rows of the
// block-column, work[i, :] <- A[i, K] and A[i, K] <- -(A[i, K] D) for i outside K.  D = A[K, K] is only read here.  A workgroup
// writes what it alone has read, after its barrier.
__global__ __launch_bounds__(kEaThreads) void ease_panel_kernel(int n, float *__restrict__ A, float *__restrict__ work, int ldw, int k0,
                                                                int bk, const int *__restrict__ status)
{
    __shared__ float sX[kEaTile][kEaLd], sY[kEaTile][kEaLd];
    if (status[0] != 0) return;
    const int nT = gridDim.x / 2;
    const bool rowp = (int)blockIdx.x < nT;
    const int t0 = kEaTile * (rowp ? (int)blockIdx.x : (int)blockIdx.x - nT);
    const int tid = threadIdx.x, c = tid & 63, r0 = tid >> 6, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
    for (int r = r0; r < kEaTile; r += 4) {
        const float d = (r < bk && c < bk) ? A[(size_t)(k0 + r) * n + k0 + c] : 0.0f;      // D[r][c]
        if (rowp) {
            sX[r][c] = d;                                                                   // i = r, k = c
            sY[c][r] = (r < bk && t0 + c < n) ? A[(size_t)(k0 + r) * n + t0 + c] : 0.0f;     // k = r, j = c
        } else {
            const bool in = t0 + r < n && c < bk;
            const float v = in ? A[(size_t)(t0 + r) * n + k0 + c] : 0.0f;                    // i = r, k = c
            sX[r][c] = v;
            if (in) work[(size_t)(t0 + r) * ldw + c] = v;
            sY[c][r] = d;                                                                   // k = r, j = c
        }
    }
    __syncthreads();
    ea_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    acc = ea_tile_mma(sX, sY, wr, wc, lane, (bk + 1) & ~1, acc);
    const int cj = wc * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ri = wr * 32 + ea_acc_row(r, lane);
        if (rowp) {
            const int j = t0 + cj;
            if (ri < bk && j < n && (j < k0 || j >= k0 + bk)) A[(size_t)(k0 + ri) * n + j] = acc[r];
        } else {
            const int i = t0 + ri;
            if (cj < bk && i < n && (i < k0 || i >= k0 + bk)) A[(size_t)i * n + k0 + cj] = -acc[r];
        }
    }
}

// Tile (blockIdx.y, blockIdx.x): A[i, j] <- A[i, j] - work[i, :] A[K, j] for i and j outside K.  The products are summed from
// zero in k order on the MFMA and subtracted once: a chain that starts from A[i, j] would round every step at the magnitude of
// A[i, j], and where the update is small against it (few raters, a large lambda) that cost up to nine times the error.
__global__ __launch_bounds__(kEaThreads) void ease_trailing_kernel(int n, float *__restrict__ A, const float *__restrict__ work, int ldw,
                                                                   int k0, int bk, const int *__restrict__ status)
{
    __shared__ float sX[kEaTile][kEaLd], sY[kEaTile][kEaLd];
    if (status[0] != 0) return;
    const int i0 = kEaTile * blockIdx.y, j0 = kEaTile * blockIdx.x;
    if ((i0 >= k0 && min(i0 + kEaTile, n) <= k0 + bk) || (j0 >= k0 && min(j0 + kEaTile, n) <= k0 + bk)) return;   // all of it inside K
    const int tid = threadIdx.x, c = tid & 63, r0 = tid >> 6, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
    for (int r = r0; r < kEaTile; r += 4) {
        sX[r][c] = (i0 + r < n && c < bk) ? work[(size_t)(i0 + r) * ldw + c] : 0.0f;         // i = r, k = c
        sY[c][r] = (r < bk && j0 + c < n) ? A[(size_t)(k0 + r) * n + j0 + c] : 0.0f;          // k = r, j = c
    }
    const int j = j0 + wc * 32 + (lane & 31);
    const bool j_ok = j < n && (j < k0 || j >= k0 + bk);
    ea_f32x16 a, acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + wr * 32 + ea_acc_row(r, lane);
        a[r] = (j_ok && i < n) ? A[(size_t)i * n + j] : 0.0f;
        acc[r] = 0.0f;
    }
    __syncthreads();
    acc = ea_tile_mma(sX, sY, wr, wc, lane, (bk + 1) & ~1, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + wr * 32 + ea_acc_row(r, lane);
        if (j_ok && i < n && (i < k0 || i >= k0 + bk)) A[(size_t)i * n + j] = a[r] - acc[r];
    }
}

RK_EXPORT int rk_ease_invert(int32_t n_items, float *A, float *work, int64_t work_floats, int32_t block, int32_t *status, void *stream)
{
    if (!A || !work || !status) RK_FAIL(RK_EINVAL, "rk_ease_invert: bad arguments");
    if (n_items < 1 || n_items > RK_EASE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_ease_invert: %d items outside 1..%d", n_items, RK_EASE_MAX_ITEMS);
    if (block != 0 && block != RK_EASE_BLOCK_SMALL && block != RK_EASE_BLOCK_LARGE)
        RK_FAIL(RK_EINVAL, "rk_ease_invert: block = %d (0, %d or %d)", block, RK_EASE_BLOCK_SMALL, RK_EASE_BLOCK_LARGE);
    const int b = block ? block : (n_items <= RK_EASE_BLOCK_SMALL ? RK_EASE_BLOCK_SMALL : RK_EASE_BLOCK_LARGE);
    if (work_floats < (int64_t)n_items * b)
        RK_FAIL(RK_EINVAL, "rk_ease_invert: a workspace of %lld floats, %lld needed (%d items x block %d)", (long long)work_floats,
                (long long)n_items * b, n_items, b);
    hipStream_t s = (hipStream_t)stream;
    int st[2] = {0, -1};
    RK_HIP(rk_set_status(status, 0, -1, s));
    const int nT = (n_items + kEaTile - 1) / kEaTile;
    for (int k0 = 0; k0 < n_items; k0 += b) {
        const int bk = std::min(b, n_items - k0);
        hipLaunchKernelGGL(ease_pivot_kernel, dim3(1), dim3(kEaThreads), 0, s, n_items, A, k0, bk, status);
        RK_CHECK_LAUNCH();
        if (n_items == bk) break;                                      // a single block: there is nothing beside it
        hipLaunchKernelGGL(ease_panel_kernel, dim3(2 * nT), dim3(kEaThreads), 0, s, n_items, A, work, b, k0, bk, status);
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(ease_trailing_kernel, dim3(nT, nT), dim3(kEaThreads), 0, s, n_items, A, work, b, k0, bk, status);
        RK_CHECK_LAUNCH();
    }
    RK_HIP(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (st[0] != 0) RK_FAIL(RK_EINVAL, "rk_ease_invert: pivot %d is not a finite positive number: the matrix is not positive definite", st[1]);
    return RK_OK;
}

// ---- weights
__global__ __launch_bounds__(256) void ease_diag_kernel(int n, const float *__restrict__ P, float *__restrict__ diag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) diag[i] = P[(size_t)i * n + i];
}

__global__ __launch_bounds__(256) void ease_weights_kernel(int n, const float *P, const float *__restrict__ diag, float *B)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double d = (double)diag[j];
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const size_t at = (size_t)i * n + j;
        B[at] = i == j ? 0.0f : -(float)((double)P[at] / d);
    }
}

RK_EXPORT int rk_ease_weights(int32_t n_items, const float *P, float *B, void *stream)
{
    if (!P || !B) RK_FAIL(RK_EINVAL, "rk_ease_weights: bad arguments");
    if (n_items < 1 || n_items > RK_EASE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_ease_weights: %d items outside 1..%d", n_items, RK_EASE_MAX_ITEMS);
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    float *diag;
    RK_HIP(scratch.get(&diag, (size_t)n_items));
    hipLaunchKernelGGL(ease_diag_kernel, dim3((n_items + 255) / 256), dim3(256), 0, s, n_items, P, diag);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(ease_weights_kernel, dim3((n_items + 255) / 256, std::min(n_items, 65535)), dim3(256), 0, s, n_items, P, diag, B);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- scores
// s + fl(q * w): two roundings, never one fused multiply-add
__device__ __forceinline__ float ea_add_term(float s, float q, float w)
{
#pragma clang fp contract(off)
    const float term = q * w;
    return s + term;
}

// Block x of the grid is one entry of user_ids, block y 256 consecutive items j, one per lane: entry e of the user's row reads row
// i_e of B as coalesced lines.  The entries are staged in LDS 256 at a time.
__global__ __launch_bounds__(256) void ease_scores_kernel(int n, const float *__restrict__ B, const int *__restrict__ rowptr,
                                                          const int *__restrict__ col, const float *__restrict__ val,
                                                          const int *__restrict__ user_ids, float *__restrict__ out)
{
    __shared__ int sc[256];
    __shared__ float sq[256];
    const int tid = threadIdx.x, j = blockIdx.y * 256 + tid;
    const int u = user_ids[blockIdx.x];
    const int beg = rowptr[u], end = rowptr[u + 1];
    float s = 0.0f;
    for (int e0 = beg; e0 < end; e0 += 256) {
        const int cnt = min(256, end - e0);
        __syncthreads();
        if (tid < cnt) {
            sc[tid] = col[e0 + tid];
            sq[tid] = (float)(int)val[e0 + tid];
        }
        __syncthreads();
        if (j < n) {
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                const int i = sc[t];
                if ((unsigned)i < (unsigned)n) s = ea_add_term(s, sq[t], B[(size_t)i * n + j]);
            }
        }
    }
    if (j < n) out[(size_t)blockIdx.x * n + j] = s;
}

RK_EXPORT int rk_ease_scores(int32_t n_items, const float *B, const int32_t *rowptr, const int32_t *col, const float *val, int32_t nb,
                             const int32_t *user_ids, float *out, void *stream)
{
    if (nb < 0 || !B || !rowptr || !col || !val) RK_FAIL(RK_EINVAL, "rk_ease_scores: bad arguments");
    if (n_items < 1 || n_items > RK_EASE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_ease_scores: %d items outside 1..%d", n_items, RK_EASE_MAX_ITEMS);
    if (nb == 0) return RK_OK;
    if (!user_ids || !out) RK_FAIL(RK_EINVAL, "rk_ease_scores: bad arguments");
    hipLaunchKernelGGL(ease_scores_kernel, dim3(nb, (n_items + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_items, B, rowptr, col, val,
                       user_ids, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// one thread per pair: the user's entries in column order
__global__ __launch_bounds__(256) void ease_pair_kernel(int n_items, int n_users, const float *__restrict__ B, const int *__restrict__ rowptr,
                                                        const int *__restrict__ col, const float *__restrict__ val,
                                                        const long long *__restrict__ users, const long long *__restrict__ items, long long n,
                                                        float *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long u = users[p], j = items[p];
    float s = 0.0f;
    if (u >= 0 && u < n_users && j >= 0 && j < n_items) {
        const int end = rowptr[u + 1];
        for (int e = rowptr[u]; e < end; ++e) {
            const int i = col[e];
            if ((unsigned)i < (unsigned)n_items) s = ea_add_term(s, (float)(int)val[e], B[(size_t)i * n_items + j]);
        }
    }
    out[p] = s;
}

RK_EXPORT int rk_ease_pair_scores(int32_t n_items, int32_t n_users, const float *B, const int32_t *rowptr, const int32_t *col,
                                  const float *val, const int64_t *users, const int64_t *items, int64_t n, float *out, void *stream)
{
    if (n_users <= 0 || n < 0 || !B || !rowptr || !col || !val) RK_FAIL(RK_EINVAL, "rk_ease_pair_scores: bad arguments");
    if (n_items < 1 || n_items > RK_EASE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_ease_pair_scores: %d items outside 1..%d", n_items, RK_EASE_MAX_ITEMS);
    if (n == 0) return RK_OK;
    if (!users || !items || !out) RK_FAIL(RK_EINVAL, "rk_ease_pair_scores: bad arguments");
    if ((n + 255) / 256 > 0x7fffffffLL) RK_FAIL(RK_EINVAL, "rk_ease_pair_scores: too many pairs");
    hipLaunchKernelGGL(ease_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_items, n_users, B, rowptr,
                       col, val, reinterpret_cast<const long long *>(users), reinterpret_cast<const long long *>(items), (long long)n, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
