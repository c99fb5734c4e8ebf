// PCASelectUsers defender (recad/model/defense/PCASelectUsers.py:47-93) on the device: the spectral fake-user
// detector's O(nnz) and O(I*b) work.  The dense U x I array and the I x I covariance the reference forms are never
// built: C.X = D^-1 A^T (A (D^-1 X)) is two narrow SpMMs over A and its transpose (rk_pca_spmm), D = diag(sigma_j)
// comes from the transposed rows (rk_pca_col_scale), and the Rayleigh-Ritz pieces are an fp64 Gram (rk_pca_gram)
// and a tall-skinny product (rk_pca_update).  Every reduction runs in a fixed order: no float atomics, so repeated
// runs are bit-identical.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.h"

// ---- transpose: radix-sort (col << 32 | row) with the values as payload; rows of A^T list users ascending
__global__ void pca_edge_keys_kernel(int n_rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                     unsigned long long *__restrict__ keys)
{
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    for (int k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64) keys[k] = ((unsigned long long)(unsigned)col[k] << 32) | (unsigned)r;
}

// t_rowptr[c] = first sorted key whose column is >= c
__global__ void pca_t_rowptr_kernel(int n_cols, long long nnz, const unsigned long long *__restrict__ keys, int *__restrict__ t_rowptr)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_cols) return;
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)(keys[mid] >> 32) < c) lo = mid + 1; else hi = mid;
    }
    t_rowptr[c] = (int)lo;
}

__global__ void pca_t_col_kernel(long long nnz, const unsigned long long *__restrict__ keys, int *__restrict__ t_col)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x)
        t_col[e] = (int)(keys[e] & 0xffffffffULL);
}

RK_EXPORT int rk_pca_transpose(int32_t n_rows, int32_t n_cols, const int32_t *rowptr, const int32_t *col, const float *val,
                               int32_t *t_rowptr, int32_t *t_col, float *t_val, void *stream)
{
    if (n_rows <= 0 || n_cols <= 0 || !rowptr || !col || !val || !t_rowptr || !t_col || !t_val)
        RK_FAIL(RK_EINVAL, "rk_pca_transpose: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    int32_t nnz = 0;
    RK_HIP(hipMemcpyAsync(&nnz, rowptr + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (nnz < 0) RK_FAIL(RK_EINVAL, "rk_pca_transpose: rowptr[n_rows] = %d", nnz);
    if (nnz == 0) {
        RK_HIP(hipMemsetAsync(t_rowptr, 0, sizeof(int32_t) * ((size_t)n_cols + 1), s));
        return RK_OK;
    }
    int end_bit = 32;
    while (end_bit < 64 && (1LL << (end_bit - 32)) < (long long)n_cols) ++end_bit;
    RkScratch scratch(s);
    unsigned long long *keys = nullptr, *sorted = nullptr;
    void *tmp_sort = nullptr;
    size_t tmp_bytes = 0;
    RK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, sorted, val, t_val, (int)nnz, 0, end_bit, s));
    RK_HIP(scratch.get(&keys, (size_t)nnz));
    RK_HIP(scratch.get(&sorted, (size_t)nnz));
    RK_HIP(scratch.bytes(&tmp_sort, tmp_bytes));
    hipLaunchKernelGGL(pca_edge_keys_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, s, n_rows, rowptr, col, keys);
    RK_CHECK_LAUNCH();
    RK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp_sort, tmp_bytes, keys, sorted, val, t_val, (int)nnz, 0, end_bit, s));
    hipLaunchKernelGGL(pca_t_rowptr_kernel, dim3((n_cols + 1 + 255) / 256), dim3(256), 0, s, n_cols, (long long)nnz, sorted, t_rowptr);
    RK_CHECK_LAUNCH();
    const int grid = (int)std::min<long long>(((long long)nnz + 255) / 256, 8192);
    hipLaunchKernelGGL(pca_t_col_kernel, dim3(grid), dim3(256), 0, s, (long long)nnz, sorted, t_col);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- column scale (sklearn.preprocessing.scale(csr, axis=0, with_mean=False)): per column j, over ALL n_users rows
// (zeros included), mean and population variance in fp64 the way sklearn's sparse mean_variance_axis sums them
// (sum over the stored entries of (x - mean)^2, plus (n - nnz) * mean^2), rounded to fp32; var < 10 * FLT_EPSILON
// counts as constant (_handle_zeros_in_scale) and gets scale 1.  One wave per row of A^T; lane-strided sums meet in a
// fixed butterfly, so the result is deterministic.
__global__ __launch_bounds__(256) void pca_col_scale_kernel(int n_cols, int n_users, const int *__restrict__ t_rowptr,
                                                            const float *__restrict__ t_val, float *__restrict__ inv_scale,
                                                            float *__restrict__ sigma)
{
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n_cols) return;
    const int b = t_rowptr[j], e = t_rowptr[j + 1];
    double s1 = 0.0;
    for (int k = b + lane; k < e; k += 64) s1 += (double)t_val[k];
    s1 = wave_sum(s1);
    const double mean = s1 / (double)n_users;
    double s2 = 0.0;
    for (int k = b + lane; k < e; k += 64) {
        const double d = (double)t_val[k] - mean;
        s2 += d * d;
    }
    s2 = wave_sum(s2);
    if (lane == 0) {
        const double var = (s2 + (double)(n_users - (e - b)) * mean * mean) / (double)n_users;
        float vf = (float)var;
        if (!(vf >= 10.0f * 1.1920928955078125e-07f)) vf = 1.0f;
        const float sd = sqrtf(vf);
        inv_scale[j] = 1.0f / sd;
        if (sigma) sigma[j] = sd;
    }
}

RK_EXPORT int rk_pca_col_scale(int32_t n_cols, int32_t n_users, const int32_t *t_rowptr, const float *t_val, float *inv_scale,
                               float *sigma, void *stream)
{
    if (n_cols <= 0 || n_users <= 0 || !t_rowptr || !t_val || !inv_scale) RK_FAIL(RK_EINVAL, "rk_pca_col_scale: bad arguments");
    hipLaunchKernelGGL(pca_col_scale_kernel, dim3((n_cols + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_cols, n_users, t_rowptr, t_val,
                       inv_scale, sigma);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- narrow SpMM  Y = diag(r_out) . A . diag(c_in) . X,  X: [n_cols, B] row-major, Y: [n_rows, B], B in {8, 16}.
// A gathered row of X is 32 or 64 B: B/4 lanes take one nonzero (one float4 each), so a wave covers 64/(B/4) nonzeros
// per step, and kUnroll steps are issued before the first is used (4 x 32 = 128 gathers of 32 B in flight per wave
// at B = 8).  One wave per output row; the lane groups' partial sums meet in a fixed xor butterfly (deterministic).
static constexpr int kPcaUnroll = 4;

template <int B, bool CIN, bool ROUT>
__global__ __launch_bounds__(256) void pca_spmm_kernel(int n_rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const float *__restrict__ val, const float *__restrict__ c_in,
                                                       const float *__restrict__ r_out, const float *__restrict__ X, float *__restrict__ Y)
{
    constexpr int LPN = B / 4, NPW = 64 / LPN;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    const int sub = lane % LPN, slot = lane / LPN;
    const int beg = rowptr[r], end = rowptr[r + 1];
    const float4 *__restrict__ X4 = reinterpret_cast<const float4 *>(X);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = beg + slot; k0 < end; k0 += kPcaUnroll * NPW) {
        int c[kPcaUnroll];
        float v[kPcaUnroll];
#pragma unroll
        for (int u = 0; u < kPcaUnroll; ++u) {
            const int k = k0 + u * NPW;
            const bool ok = k < end;
            c[u] = ok ? col[k] : 0;
            v[u] = ok ? val[k] : 0.f;
        }
        float4 x[kPcaUnroll];
#pragma unroll
        for (int u = 0; u < kPcaUnroll; ++u) {
            x[u] = X4[(size_t)c[u] * LPN + sub];
            if (CIN) v[u] *= c_in[c[u]];
        }
#pragma unroll
        for (int u = 0; u < kPcaUnroll; ++u) {
            acc.x += v[u] * x[u].x;
            acc.y += v[u] * x[u].y;
            acc.z += v[u] * x[u].z;
            acc.w += v[u] * x[u].w;
        }
    }
#pragma unroll
    for (int o = LPN; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o, 64);
        acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64);
        acc.w += __shfl_xor(acc.w, o, 64);
    }
    if (slot == 0) {
        const float sc = ROUT ? r_out[r] : 1.0f;
        reinterpret_cast<float4 *>(Y)[(size_t)r * LPN + sub] = make_float4(acc.x * sc, acc.y * sc, acc.z * sc, acc.w * sc);
    }
}

template <int B>
static void launch_pca_spmm(int n_rows, const int *rowptr, const int *col, const float *val, const float *c_in, const float *r_out,
                            const float *X, float *Y, hipStream_t s)
{
    const dim3 grid((n_rows + 3) / 4), block(256);
    if (c_in && r_out) hipLaunchKernelGGL((pca_spmm_kernel<B, true, true>), grid, block, 0, s, n_rows, rowptr, col, val, c_in, r_out, X, Y);
    else if (c_in) hipLaunchKernelGGL((pca_spmm_kernel<B, true, false>), grid, block, 0, s, n_rows, rowptr, col, val, c_in, r_out, X, Y);
    else if (r_out) hipLaunchKernelGGL((pca_spmm_kernel<B, false, true>), grid, block, 0, s, n_rows, rowptr, col, val, c_in, r_out, X, Y);
    else hipLaunchKernelGGL((pca_spmm_kernel<B, false, false>), grid, block, 0, s, n_rows, rowptr, col, val, c_in, r_out, X, Y);
}

RK_EXPORT int rk_pca_spmm(int32_t n_rows, const int32_t *rowptr, const int32_t *col, const float *val, const float *c_in,
                          const float *r_out, int32_t b, const float *X, float *Y, void *stream)
{
    if (n_rows <= 0 || !rowptr || !col || !val || !X || !Y) RK_FAIL(RK_EINVAL, "rk_pca_spmm: bad arguments");
    if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) RK_FAIL(RK_EINVAL, "rk_pca_spmm: X / Y not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (b == 8) launch_pca_spmm<8>(n_rows, rowptr, col, val, c_in, r_out, X, Y, s);
    else if (b == 16) launch_pca_spmm<16>(n_rows, rowptr, col, val, c_in, r_out, X, Y, s);
    else RK_FAIL(RK_EINVAL, "rk_pca_spmm: block width %d (supported: 8, 16)", b);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- dist = (A o A) . w,  w[j] = sum_{c < k} V[j, c]  (PCASelectUsers.py:68-78: the raw squared ratings times the sum of
// the k eigenvectors).  w is built first (fixed column order); the SpMV accumulates in fp64, one wave per row.
__global__ void pca_vec_sum_kernel(int n, const float *__restrict__ V, int ldv, int k, float *__restrict__ w)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int c = 0; c < k; ++c) s += (double)V[(size_t)j * ldv + c];
    w[j] = (float)s;
}

__global__ __launch_bounds__(256) void pca_sq_spmv_kernel(int n_rows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                          const float *__restrict__ val, const float *__restrict__ w, float *__restrict__ dist)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    double s = 0.0;
    for (int k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64) {
        const double a = (double)val[k];
        s += a * a * (double)w[col[k]];
    }
    s = wave_sum(s);
    if (lane == 0) dist[r] = (float)s;
}

RK_EXPORT int rk_pca_sq_spmv(int32_t n_rows, int32_t n_cols, const int32_t *rowptr, const int32_t *col, const float *val, const float *V,
                             int32_t ldv, int32_t k, float *w, float *dist, void *stream)
{
    if (n_rows <= 0 || n_cols <= 0 || k <= 0 || ldv < k || !rowptr || !col || !val || !V || !w || !dist)
        RK_FAIL(RK_EINVAL, "rk_pca_sq_spmv: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_vec_sum_kernel, dim3((n_cols + 255) / 256), dim3(256), 0, s, n_cols, V, ldv, k, w);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pca_sq_spmv_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, s, n_rows, rowptr, col, val, w, dist);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- Gram G = Z^T Z of Z = [P | Q] (n x (p + q), both row-major, Q optional) in fp64.  RK_PCA_GRAM_BLOCKS workgroups
// each own a fixed contiguous row range and write their (p+q)^2 partial sums; a second kernel adds the partials in block
// order.  The result depends on n only, never on timing.
static constexpr int kGramTile = 64;

__global__ __launch_bounds__(256) void pca_gram_partial_kernel(long long n, const float *__restrict__ P, int p, const float *__restrict__ Q,
                                                               int q, double *__restrict__ part)
{
    __shared__ float tile[kGramTile][33];
    const int w = p + q, ww = w * w, tid = threadIdx.x;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long r0 = (long long)blockIdx.x * per, r1 = std::min(n, r0 + per);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long t0 = r0; t0 < r1; t0 += kGramTile) {
        const int rows = (int)std::min<long long>(kGramTile, r1 - t0);
        for (int e = tid; e < rows * w; e += 256) {
            const int rr = e / w, c = e % w;
            const long long g = t0 + rr;
            tile[rr][c] = c < p ? P[g * p + c] : Q[g * q + (c - p)];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int o = tid + s * 256;
            if (o < ww) {
                const int i = o / w, j = o % w;
                double a = acc[s];
                for (int rr = 0; rr < rows; ++rr) a += (double)tile[rr][i] * (double)tile[rr][j];
                acc[s] = a;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int o = tid + s * 256;
        if (o < ww) part[(size_t)blockIdx.x * ww + o] = acc[s];
    }
}

__global__ void pca_gram_sum_kernel(int nb, int ww, const double *__restrict__ part, double *__restrict__ G)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= ww) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(size_t)b * ww + o];
    G[o] = s;
}

RK_EXPORT int rk_pca_gram(int64_t n, const float *P, int32_t p, const float *Q, int32_t q, double *part, double *G, void *stream)
{
    if (n <= 0 || !P || p <= 0 || q < 0 || (q > 0 && !Q) || p + q > 32 || !part || !G) RK_FAIL(RK_EINVAL, "rk_pca_gram: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int ww = (p + q) * (p + q);
    hipLaunchKernelGGL(pca_gram_partial_kernel, dim3(RK_PCA_GRAM_BLOCKS), dim3(256), 0, s, (long long)n, P, p, Q, q, part);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pca_gram_sum_kernel, dim3((ww + 255) / 256), dim3(256), 0, s, RK_PCA_GRAM_BLOCKS, ww, part, G);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- V_out = V . M,  V: [n, p] fp32 row-major, M: [p, q] fp64 row-major (device), accumulated in fp64
__global__ __launch_bounds__(256) void pca_update_kernel(long long n, const float *__restrict__ V, int p, const double *__restrict__ M, int q,
                                                         float *__restrict__ out)
{
    __shared__ double m[32 * 32];
    for (int e = threadIdx.x; e < p * q; e += blockDim.x) m[e] = M[e];
    __syncthreads();
    const long long total = n * q;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const long long r = o / q;
        const int c = (int)(o % q);
        double s = 0.0;
        for (int k = 0; k < p; ++k) s += (double)V[r * p + k] * m[k * q + c];
        out[o] = (float)s;
    }
}

RK_EXPORT int rk_pca_update(int64_t n, const float *V, int32_t p, const double *M, int32_t q, float *out, void *stream)
{
    if (n <= 0 || !V || !M || !out || p <= 0 || q <= 0 || p > 32 || q > 32 || V == out) RK_FAIL(RK_EINVAL, "rk_pca_update: bad arguments");
    const int grid = (int)std::min<long long>((n * q + 255) / 256, 8192);
    hipLaunchKernelGGL(pca_update_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)n, V, p, M, q, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- selection: the m smallest (dist, id) pairs in Python's stable ascending sort order (PCASelectUsers.py:80-90).
// Key = order-preserving encoding of the fp32 distance in the high 32 bits, the user id in the low 32: one radix sort
// gives ties to the lower id, exactly like sorted(..., key=dist).  Non-finite distances are counted and refused.
// `largest`: the encoding is complemented, so the same ascending sort lists the largest first, ties still to the lower id.
__global__ void pca_select_keys_kernel(int n, const float *__restrict__ dist, int largest, unsigned long long *__restrict__ keys,
                                       int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d = dist[i];
    if (!isfinite(d)) atomicAdd(bad, 1);
    if (d == 0.0f) d = 0.0f;    // -0 and +0 compare equal in Python: one key
    unsigned u = __float_as_uint(d);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (largest) u = ~u;
    keys[i] = ((unsigned long long)u << 32) | (unsigned)i;
}

__global__ void pca_select_out_kernel(int m, const unsigned long long *__restrict__ sorted, int *__restrict__ ids)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) ids[i] = (int)(sorted[i] & 0xffffffffULL);
}

// shared by rk_pca_select and rk_knn_select (declared in common.h)
int rk_select_ids(const char *who, const char *noun, int32_t n, const float *dist, int32_t m, int32_t largest, int32_t *order, void *stream)
{
    if (n <= 0 || m < 0 || m > n || !dist || !order) RK_FAIL(RK_EINVAL, "%s: bad arguments", who);
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *keys = nullptr, *sorted = nullptr;
    int *bad = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, keys, sorted, n, 0, 64, s));
    RK_HIP(scratch.get(&keys, (size_t)n));
    RK_HIP(scratch.get(&sorted, (size_t)n));
    RK_HIP(scratch.get(&bad, 1));
    RK_HIP(scratch.bytes(&tmp, tmp_bytes));
    RK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    hipLaunchKernelGGL(pca_select_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, dist, largest, keys, bad);
    RK_CHECK_LAUNCH();
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, keys, sorted, n, 0, 64, s));
    if (m > 0) {
        hipLaunchKernelGGL(pca_select_out_kernel, dim3((m + 255) / 256), dim3(256), 0, s, m, sorted, order);
        RK_CHECK_LAUNCH();
    }
    int h_bad = 0;
    RK_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (h_bad) RK_FAIL(RK_EINVAL, "%s: %d non-finite %s", who, h_bad, noun);
    return RK_OK;
}

RK_EXPORT int rk_pca_select(int32_t n, const float *dist, int32_t m, int32_t *order, void *stream)
{
    return rk_select_ids("rk_pca_select", "distances", n, dist, m, 0, order, stream);
}
