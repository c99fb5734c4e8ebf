// CatchSyncSelectUsers defender: synchronicity of a user's items over a grid of item features (Jiang, Cui, Beutel, Faloutsos,
// Yang, "CatchSync", KDD 2014), integer-exact: item degree and reach (one HITS step from the all-ones hub vector), half-octave
// style buckets by shifts and masks, cells = the distinct (degree bucket, reach bucket) keys in ascending order, per-user
// pair and background sums in int64 from an int32 histogram in LDS (integer LDS atomics: exact in any arrival order), and
// the three scores in fp64 from those integers.  include/recad_hip.h states the definition.
#include <limits.h>

#include "common.h"

static constexpr int kCsKeys = 65536;          // compact key bucket(deg) * 256 + bucket(reach): both buckets are below 256 at s = 3
static constexpr int kCsLongRow = 512;         // form 0: a longer row is walked by the whole workgroup
static constexpr int kCsWaveUsers = 32;        // `order` entries per workgroup where waves take users (8 in turn per wave)
static constexpr int kCsGroupUsers = 8;        // entries per workgroup where the workgroup takes one user at a time
static_assert(4 * 4 * RK_CS_MAX_CELLS + 64 <= kLdsMaxBytes, "four histogram slices do not fit a CU's LDS");

// x >= 1: e = index of the leading one, m = the s bits below it (zero-filled when e < s); e * 2^s + m
__device__ __forceinline__ int cs_bucket(int x, int s)
{
    const int e = 31 - __clz(x);
    const int m = (e >= s ? (x >> (e - s)) : (x << (s - e))) & ((1 << s) - 1);
    return (e << s) + m;
}

// ---- features: one wave per item
__global__ __launch_bounds__(256) void cs_features_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                          const int *__restrict__ colptr, const int *__restrict__ crow,
                                                          int *__restrict__ deg_item, int *__restrict__ reach)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n_items) return;
    const int beg = colptr[i], end = colptr[i + 1];
    int r = 0;
    for (int p = beg + lane; p < end; p += 64) {
        const int u = crow[p];
        if ((unsigned)u < (unsigned)n_users) r += rowptr[u + 1] - rowptr[u];
    }
    r = wave_sum(r);
    if (lane == 0) {
        deg_item[i] = end - beg;
        reach[i] = r;
    }
}

RK_EXPORT int rk_cs_features(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *colptr, const int32_t *crow,
                             int32_t *deg_item, int32_t *reach, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || !rowptr || !colptr || !crow || !deg_item || !reach) RK_FAIL(RK_EINVAL, "rk_cs_features: bad arguments");
    hipLaunchKernelGGL(cs_features_kernel, dim3((n_items + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_users, n_items, rowptr, colptr,
                       crow, deg_item, reach);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- cells
__global__ __launch_bounds__(256) void cs_keys_kernel(int n_items, const int *__restrict__ deg_item, const int *__restrict__ reach, int s,
                                                      int *__restrict__ key, int *__restrict__ cnt, unsigned long long *__restrict__ first_bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int d = deg_item[i], r = reach[i];
    int k = -1;
    if (d < 0 || r < 0 || (d > 0 && r == 0)) {
        rk_record_bad(first_bad, i, RK_CS_BAD_FEATURE);
    } else if (d > 0) {
        k = cs_bucket(d, s) * 256 + cs_bucket(r, s);
        atomicAdd(&cnt[k], 1);
    }
    key[i] = k;
}

// One workgroup: rank[k] = the number of present keys below k (-1 for an absent key), cell_count[rank] = cnt, info.
__global__ __launch_bounds__(256) void cs_rank_kernel(const int *__restrict__ cnt, int *__restrict__ rank, int *__restrict__ cell_count,
                                                      long long *__restrict__ info)
{
    __shared__ int part[256];
    __shared__ long long red[4];
    __shared__ int lo_hi[2], m_total;
    const int tid = threadIdx.x, k0 = tid * (kCsKeys / 256);
    for (int j = tid; j < RK_CS_MAX_CELLS; j += 256) cell_count[j] = 0;
    if (tid == 0) { lo_hi[0] = INT_MAX; lo_hi[1] = 0; }
    int own = 0;
    for (int b = 0; b < kCsKeys / 256; ++b) own += cnt[k0 + b] > 0;
    part[tid] = own;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { const int c = part[t]; part[t] = run; run += c; }
    }
    __syncthreads();
    int r = part[tid], mn = INT_MAX, mx = 0;
    long long n = 0, sb = 0;
    for (int b = 0; b < kCsKeys / 256; ++b) {
        const int c = cnt[k0 + b];
        if (c > 0) {
            rank[k0 + b] = r;
            if (r < RK_CS_MAX_CELLS) cell_count[r] = c;
            n += c;
            sb += (long long)c * c;
            mn = min(mn, c);
            mx = max(mx, c);
            ++r;
        } else {
            rank[k0 + b] = -1;
        }
    }
    if (mx > 0) { atomicMin(&lo_hi[0], mn); atomicMax(&lo_hi[1], mx); }
    if (tid == 255) m_total = r;                                       // the last thread's running rank is M
    n = block_sum_256(n, red);
    sb = block_sum_256(sb, red);
    if (tid == 0) {
        info[0] = m_total;
        info[1] = n;
        info[2] = sb;
        info[3] = (m_total == 0 || lo_hi[0] == lo_hi[1]) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void cs_assign_kernel(int n_items, const int *__restrict__ key, const int *__restrict__ rank,
                                                        int *__restrict__ cell_of, unsigned long long *__restrict__ first_bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int k = key[i];
    const int c = k < 0 ? -1 : rank[k];
    if (c >= RK_CS_MAX_CELLS) rk_record_bad(first_bad, i, RK_CS_TOO_MANY_CELLS);
    cell_of[i] = c;
}

RK_EXPORT int rk_cs_cells(int32_t n_items, const int32_t *deg_item, const int32_t *reach, int32_t grid_bits, int32_t *cell_of,
                          int32_t *cell_count, int64_t *info, int32_t *status, void *stream)
{
    if (n_items <= 0 || !deg_item || !reach || !cell_of || !cell_count || !info || !status) RK_FAIL(RK_EINVAL, "rk_cs_cells: bad arguments");
    if (n_items >= RK_CS_MAX_ITEMS) RK_FAIL(RK_EINVAL, "rk_cs_cells: n_items = %d, at most 2^26 - 1", n_items);
    if (grid_bits < 0 || grid_bits > 3) RK_FAIL(RK_EINVAL, "rk_cs_cells: grid_bits = %d outside 0..3", grid_bits);
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *first_bad = nullptr;
    int *tab = nullptr, *key = nullptr, *cell_tmp = nullptr, *count_tmp = nullptr;     // tab: cnt[kCsKeys] | rank[kCsKeys]
    long long *info_tmp = nullptr;
    RK_HIP(scratch.get(&first_bad, 1));
    RK_HIP(scratch.get(&tab, (size_t)2 * kCsKeys));
    RK_HIP(scratch.get(&key, (size_t)n_items));
    RK_HIP(scratch.get(&cell_tmp, (size_t)n_items));
    RK_HIP(scratch.get(&count_tmp, (size_t)RK_CS_MAX_CELLS));
    RK_HIP(scratch.get(&info_tmp, 4));
    RK_HIP(rk_first_bad_arm(first_bad, 1, s));
    RK_HIP(rk_zero_async(tab, sizeof(int) * (size_t)kCsKeys, s));
    const int grid = (n_items + 255) / 256;
    hipLaunchKernelGGL(cs_keys_kernel, dim3(grid), dim3(256), 0, s, n_items, deg_item, reach, grid_bits, key, tab, first_bad);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(cs_rank_kernel, dim3(1), dim3(256), 0, s, tab, tab + kCsKeys, count_tmp, info_tmp);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(cs_assign_kernel, dim3(grid), dim3(256), 0, s, n_items, key, tab + kCsKeys, cell_tmp, first_bad);
    RK_CHECK_LAUNCH();
    RK_HIP(rk_first_bad_status(first_bad, 1, status, s));
    int32_t h[2] = {0, 0};
    RK_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (h[0]) {
        const char *what = h[0] == RK_CS_BAD_FEATURE ? "a negative deg_item or reach, or a rated item with reach 0"
                                                      : "more than RK_CS_MAX_CELLS cells";
        RK_FAIL(RK_EINVAL, "rk_cs_cells: rule %d (%s), first at item %d", h[0], what, h[1]);
    }
    RK_HIP(hipMemcpyAsync(cell_of, cell_tmp, sizeof(int32_t) * (size_t)n_items, hipMemcpyDeviceToDevice, s));
    RK_HIP(hipMemcpyAsync(cell_count, count_tmp, sizeof(int32_t) * (size_t)RK_CS_MAX_CELLS, hipMemcpyDeviceToDevice, s));
    RK_HIP(hipMemcpyAsync(info, info_tmp, sizeof(int64_t) * 4, hipMemcpyDeviceToDevice, s));
    return RK_OK;
}

// ---- per-user sums.  Workgroup g of G owns the entries g, g + G, g + 2 G ... of `order` (`per_wg` of them): interleaved, so
// that the long rows at the head of a descending order spread over all workgroups and each starts with its longest.  Rows of at most long_row items: one wave per
// user, wave w on its own M-word slice of the histogram; longer rows: the whole workgroup per user on slice 0, which the wave
// phase has left zero.  Per user three walks of the row: add 1 to each touched cell, read the counts back and sum them, zero
// the touched cells -- so the histogram is cleared in full once per workgroup only.
__device__ __forceinline__ void cs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");             // the wave's LDS operations so far have completed
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void cs_user_sums_kernel(int n_users, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                           const int *__restrict__ cell_of, const int *__restrict__ cell_count, int n_cells,
                                                           int long_row, int per_wg, const int *__restrict__ order,
                                                           long long *__restrict__ pair_num, long long *__restrict__ back_num)
{
    extern __shared__ int cs_hist[];
    __shared__ long long red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_words = (long_row < 0 ? 1 : 4) * n_cells;
    for (int j = tid; j < n_words; j += 256) cs_hist[j] = 0;
    __syncthreads();
    const int first = blockIdx.x, step = gridDim.x;
    if (long_row >= 0) {
        int *h = cs_hist + wave * n_cells;
#pragma unroll 1
        for (int j = wave; j < per_wg; j += 4) {
            const int b = first + j * step;
            if (b >= n_users) break;
            const int u = order ? order[b] : b;
            if (u < 0 || u >= n_users) continue;                       // `order` is not a permutation: nothing is written for this entry
            const int beg = rowptr[u], end = rowptr[u + 1];
            if (end - beg > long_row) continue;
            long long pn = 0, bn = 0;
            for (int e = beg + lane; e < end; e += 64) {
                const int c = cell_of[col[e]];
                if ((unsigned)c < (unsigned)n_cells) {
                    atomicAdd(&h[c], 1);
                    bn += cell_count[c];
                }
            }
            cs_wave_sync();
            for (int e = beg + lane; e < end; e += 64) {
                const int c = cell_of[col[e]];
                if ((unsigned)c < (unsigned)n_cells) pn += h[c];
            }
            cs_wave_sync();
            for (int e = beg + lane; e < end; e += 64) {
                const int c = cell_of[col[e]];
                if ((unsigned)c < (unsigned)n_cells) h[c] = 0;
            }
            cs_wave_sync();
            pn = wave_sum(pn);
            bn = wave_sum(bn);
            if (lane == 0) {
                pair_num[u] = pn;
                back_num[u] = bn;
            }
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < per_wg; ++j) {
        const int b = first + j * step;                                // the same for every thread of the workgroup, and so are u and the row
        if (b >= n_users) break;
        const int u = order ? order[b] : b;
        if (u < 0 || u >= n_users) continue;
        const int beg = rowptr[u], end = rowptr[u + 1];
        if (end - beg <= long_row) continue;
        long long pn = 0, bn = 0;
        for (int e = beg + tid; e < end; e += 256) {
            const int c = cell_of[col[e]];
            if ((unsigned)c < (unsigned)n_cells) {
                atomicAdd(&cs_hist[c], 1);
                bn += cell_count[c];
            }
        }
        __syncthreads();
        for (int e = beg + tid; e < end; e += 256) {
            const int c = cell_of[col[e]];
            if ((unsigned)c < (unsigned)n_cells) pn += cs_hist[c];
        }
        __syncthreads();
        for (int e = beg + tid; e < end; e += 256) {
            const int c = cell_of[col[e]];
            if ((unsigned)c < (unsigned)n_cells) cs_hist[c] = 0;
        }
        pn = block_sum_256(pn, red);                                   // its barriers also order the zeroing before the next user's adds
        bn = block_sum_256(bn, red);
        if (tid == 0) {
            pair_num[u] = pn;
            back_num[u] = bn;
        }
    }
}

RK_EXPORT int rk_cs_user_sums(int32_t n_users, const int32_t *rowptr, const int32_t *col, const int32_t *cell_of, const int32_t *cell_count,
                              int32_t n_cells, int32_t form, const int32_t *order, int64_t *pair_num, int64_t *back_num, void *stream)
{
    if (n_users <= 0 || !rowptr || !col || !cell_of || !cell_count || !pair_num || !back_num) RK_FAIL(RK_EINVAL, "rk_cs_user_sums: bad arguments");
    if (n_cells < 1 || n_cells > RK_CS_MAX_CELLS) RK_FAIL(RK_EINVAL, "rk_cs_user_sums: M = %d outside 1..%d", n_cells, RK_CS_MAX_CELLS);
    if (form < RK_CS_FORM_AUTO || form > RK_CS_FORM_WORKGROUP) RK_FAIL(RK_EINVAL, "rk_cs_user_sums: form = %d outside 0..2", form);
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cs_user_sums_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   4 * 4 * RK_CS_MAX_CELLS));
        attr_once.done(attr_dev);
    }
    const int long_row = form == RK_CS_FORM_WAVE ? INT_MAX : (form == RK_CS_FORM_WORKGROUP ? -1 : kCsLongRow);
    const int per_wg = form == RK_CS_FORM_WORKGROUP ? kCsGroupUsers : kCsWaveUsers;
    const size_t lds = (size_t)4 * n_cells * (form == RK_CS_FORM_WORKGROUP ? 1 : 4);
    hipLaunchKernelGGL(cs_user_sums_kernel, dim3((n_users + per_wg - 1) / per_wg), dim3(256), lds, (hipStream_t)stream, n_users, rowptr, col,
                       cell_of, cell_count, n_cells, long_row, per_wg, order, reinterpret_cast<long long *>(pair_num),
                       reinterpret_cast<long long *>(back_num));
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- scores: fp64 from the exact integers, every operation rounded on its own, one rounding to fp32
__global__ __launch_bounds__(256) void cs_scores_kernel(int n_users, const int *__restrict__ rowptr, const long long *__restrict__ pair_num,
                                                        const long long *__restrict__ back_num, const long long *__restrict__ info, int mode,
                                                        int min_items, float *__restrict__ score)
{
#pragma clang fp contract(off)
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n_users) return;
    const int di = rowptr[u + 1] - rowptr[u];
    if (di < min_items) {
        score[u] = -1.0f;
        return;
    }
    const double d = (double)di, p = (double)pair_num[u], bk = (double)back_num[u];
    const double M = (double)info[0], N = (double)info[1], SB = (double)info[2];
    double r;
    if (mode == RK_CS_SCORE_SYNC) {
        r = (p - d) / (d * (d - 1.0));
    } else if (mode == RK_CS_SCORE_NORMALITY) {
        r = bk / (d * N);
    } else {
        const double sy = p / (d * d), n = bk / (d * N);
        double s_min;
        if (info[3] != 0) {
            s_min = 1.0 / M;
        } else {
            const double s_b = SB / (N * N);
            s_min = (((M * n) * n - 2.0 * n) + s_b) / (M * s_b - 1.0);
        }
        r = sy - s_min;
    }
    score[u] = (float)r;
}

RK_EXPORT int rk_cs_scores(int32_t n_users, const int32_t *rowptr, const int64_t *pair_num, const int64_t *back_num, const int64_t *info,
                           int32_t mode, int32_t min_items, float *score, void *stream)
{
    if (n_users <= 0 || !rowptr || !pair_num || !back_num || !info || !score) RK_FAIL(RK_EINVAL, "rk_cs_scores: bad arguments");
    if (mode < RK_CS_SCORE_SYNC || mode > RK_CS_SCORE_RESIDUAL) RK_FAIL(RK_EINVAL, "rk_cs_scores: mode = %d outside 0..2", mode);
    if (min_items < 2) RK_FAIL(RK_EINVAL, "rk_cs_scores: min_items = %d below 2", min_items);
    hipLaunchKernelGGL(cs_scores_kernel, dim3((n_users + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_users, rowptr,
                       reinterpret_cast<const long long *>(pair_num), reinterpret_cast<const long long *>(back_num),
                       reinterpret_cast<const long long *>(info), mode, min_items, score);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
