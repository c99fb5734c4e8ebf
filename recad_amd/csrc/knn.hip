// KnnSelectUsers defender: DegSim, a profile's mean cosine similarity to its k nearest neighbours (Chirita et al. 2005;
// Burke / Mobasher et al. 2006), from the U x I rating CSR and its transpose (rk_pca_transpose).  No U x U matrix is
// formed: one workgroup per user u accumulates the integer dots d_uv of a band of candidate users in LDS (integer adds:
// the sums do not depend on arrival order, so the result is exact and repeatable), turns the nonzero ones into
// w_uv = ((float)d_uv * r_u) * r_v and folds them into a running top-k of VALUES by a radix select over their bit
// patterns (non-negative floats order as unsigned integers).  include/recad_hip.h states the definition.
#include <algorithm>

#include "common.h"

static constexpr int kKnnThreads = 256;
static constexpr int kKnnBins = 2048;                           // histogram of one radix digit (11 bits at most)
static constexpr int kKnnMisc = 16;                             // words handed between the scan wave and the block
// LDS of one workgroup: int32 acc[band] | uint32 top[RK_KNN_MAX_K] | uint32 hist[kKnnBins] | uint32 misc[kKnnMisc]
static constexpr int kKnnScratchBytes = 4 * (RK_KNN_MAX_K + kKnnBins + kKnnMisc);
static_assert(4 * RK_KNN_MAX_BAND + kKnnScratchBytes <= kLdsMaxBytes - 64, "RK_KNN_MAX_BAND does not fit a CU's LDS");
static_assert(RK_KNN_MAX_BAND % 64 == 0 && RK_KNN_MAX_K == 128, "the final sort is written for 128 slots");
static constexpr int kKnnAutoBand = 8192;                       // automatic band: 41 KiB per workgroup, 3 workgroups per CU

// ---- norms and validation: one wave per row.  First offending (row, rule) by rk_record_bad.
__global__ __launch_bounds__(256) void knn_norms_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                        const int *__restrict__ col, const float *__restrict__ val,
                                                        float *__restrict__ rnorm, unsigned long long *__restrict__ first_bad)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n_users) return;
    const int beg = rowptr[r], end = rowptr[r + 1];
    int rule = 0;
    long long n = 0;
    if (beg < 0 || end < beg) {
        rule = RK_KNN_BAD_ROWPTR;
    } else {
        bool bad_val = false, bad_col = false;
        for (int e = beg + lane; e < end; e += 64) {
            const float x = val[e];
            // 1 <= x <= 127 is false for NaN; inside that range (float)(int)x == x exactly when x is an integer
            if (!(x >= 1.0f && x <= 127.0f) || (float)(int)x != x) bad_val = true;
            else n += (long long)((int)x * (int)x);
            const int c = col[e];
            if (c < 0 || c >= n_items || (e > beg && col[e - 1] >= c)) bad_col = true;
        }
        n = wave_sum(n);
        const bool any_val = __any(bad_val), any_col = __any(bad_col);
        if (any_val) rule = RK_KNN_BAD_VALUE;
        else if (any_col) rule = RK_KNN_BAD_COLUMN;
        else if (n >= (1LL << 31)) rule = RK_KNN_BAD_NORM;
    }
    if (lane != 0) return;
    if (rule) {
        rk_record_bad(first_bad, r, rule);
        return;
    }
    rnorm[r] = n > 0 ? (float)(1.0 / sqrt((double)n)) : 0.0f;      // fp64 sqrt and divide are correctly rounded (hipcc's default)
}

RK_EXPORT int rk_knn_norms(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val, float *rnorm,
                           int32_t *status, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || !rowptr || !col || !val || !rnorm || !status) RK_FAIL(RK_EINVAL, "rk_knn_norms: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *first_bad = nullptr;
    float *tmp = nullptr;
    RK_HIP(scratch.get(&first_bad, 1));
    RK_HIP(scratch.get(&tmp, (size_t)n_users));
    RK_HIP(rk_first_bad_arm(first_bad, 1, s));
    hipLaunchKernelGGL(knn_norms_kernel, dim3((n_users + 3) / 4), dim3(256), 0, s, n_users, n_items, rowptr, col, val, tmp, first_bad);
    RK_CHECK_LAUNCH();
    RK_HIP(rk_first_bad_status(first_bad, 1, status, s));
    int32_t h[2] = {0, 0};
    RK_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (h[0]) {
        static const char *const what[] = {"", "a value that is not an integer in 1..127", "column ids not strictly ascending inside [0, n_items)",
                                           "a squared norm of 2^31 or more", "row pointers that decrease or are negative"};
        RK_FAIL(RK_EINVAL, "rk_knn_norms: rule %d (%s), first in row %d", h[0], what[h[0] <= 4 ? h[0] : 0], h[1]);
    }
    RK_HIP(hipMemcpyAsync(rnorm, tmp, sizeof(float) * (size_t)n_users, hipMemcpyDeviceToDevice, s));
    return RK_OK;
}

// ---- DegSim
// The kk-th largest bit pattern T among the nonzero words >= floor_ of acc[0, n_acc) and top[0, kk), by three radix digits
// (bits 29..19, 18..8, 7..0: every w is below 2, so bits 31 and 30 are clear), then top[0, kk) = the words above T and as
// many copies of T as it takes.  Fewer than kk such words: T = 0 and the list is padded with zeros.  Returns T (the next
// band's floor: a word below the kk-th largest so far can never enter the list).  All threads of the block call it.
__device__ unsigned knn_fold(unsigned *acc, int n_acc, unsigned *top, unsigned *hist, unsigned *misc, int kk, unsigned floor_)
{
    const int tid = threadIdx.x;
    unsigned prefix = 0, mask = 0;
    int need = kk;
    bool short_list = false;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 19 : (pass == 1 ? 8 : 0);
        const int nb = pass == 2 ? 256 : kKnnBins;
        for (int b = tid; b < nb; b += kKnnThreads) hist[b] = 0;
        __syncthreads();
        for (int j = tid; j < n_acc + kk; j += kKnnThreads) {
            const unsigned b = j < n_acc ? acc[j] : top[j - n_acc];
            if (b != 0 && b >= floor_ && (b & mask) == prefix) atomicAdd(&hist[(b >> shift) & (unsigned)(nb - 1)], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            // lane l owns bins [l * per, (l + 1) * per); suffix sums over the lanes locate the bin where the count from the top reaches `need`
            const int per = nb / 64;
            unsigned own = 0;
            for (int b = 0; b < per; ++b) own += hist[tid * per + b];
            unsigned suf = own;                                        // inclusive sum over lanes >= tid
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned t = __shfl_down(suf, o, 64);
                if (tid + o < 64) suf += t;
            }
            const unsigned total = __shfl(suf, 0, 64);
            if (tid == 0) misc[2] = total;
            if (total >= (unsigned)need && suf >= (unsigned)need && suf - own < (unsigned)need) {
                unsigned cum = suf - own;
                for (int b = per - 1; b >= 0; --b) {
                    const unsigned c = hist[tid * per + b];
                    if (cum + c >= (unsigned)need) {
                        misc[0] = (unsigned)(tid * per + b);
                        misc[1] = (unsigned)need - cum;
                        break;
                    }
                    cum += c;
                }
            }
        }
        __syncthreads();
        if (pass == 0 && misc[2] < (unsigned)need) { short_list = true; }
        if (!short_list) {
            prefix |= misc[0] << shift;
            mask |= (unsigned)(nb - 1) << shift;
            need = (int)misc[1];
        }
        __syncthreads();                                               // misc and hist are rewritten by the next pass
        if (short_list) break;
    }
    const unsigned T = short_list ? 0u : prefix;
    // gather the words above T into hist[0, kk) (any order: the list is sorted once, at the end)
    if (tid == 0) misc[3] = 0;
    __syncthreads();
    for (int j = tid; j < n_acc + kk; j += kKnnThreads) {
        const unsigned b = j < n_acc ? acc[j] : top[j - n_acc];
        if (b > T && b >= floor_) {
            const unsigned pos = atomicAdd(&misc[3], 1u);
            if (pos < (unsigned)kk) hist[pos] = b;
        }
    }
    __syncthreads();
    const unsigned n_gt = min(misc[3], (unsigned)kk);
    for (int j = tid; j < kk; j += kKnnThreads) top[j] = (unsigned)j < n_gt ? hist[j] : T;
    __syncthreads();
    return T;
}

__global__ __launch_bounds__(kKnnThreads) void knn_degsim_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                                 const int *__restrict__ col, const float *__restrict__ val,
                                                                 const int *__restrict__ colptr, const int *__restrict__ crow,
                                                                 const float *__restrict__ cval, const float *__restrict__ rnorm, int k,
                                                                 int band, const int *__restrict__ order, float *__restrict__ topw,
                                                                 float *__restrict__ degsim)
{
    extern __shared__ unsigned knn_lds[];
    unsigned *acc = knn_lds, *top = knn_lds + band, *hist = top + RK_KNN_MAX_K, *misc = hist + kKnnBins;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = order ? order[blockIdx.x] : (int)blockIdx.x;
    if (u < 0 || u >= n_users) return;                                 // `order` is not a permutation: nothing is written for this entry
    const int kk = min(k, n_users - 1);
    for (int j = tid; j < RK_KNN_MAX_K; j += kKnnThreads) top[j] = 0;
    const int beg = rowptr[u], end = rowptr[u + 1];
    const float ru = rnorm[u];
    unsigned floor_ = 0;
    if (kk > 0 && end > beg) {
#pragma unroll 1
        for (int lo = 0; lo < n_users; lo += band) {
            const int bn = min(band, n_users - lo);
            for (int j = tid; j < bn; j += kKnnThreads) acc[j] = 0;
            __syncthreads();
            const bool whole = lo == 0 && bn == n_users;
            for (int e = beg + wave; e < end; e += kKnnThreads / 64) {
                const int i = col[e];
                if (i < 0 || i >= n_items) continue;
                const int q = (int)val[e];
                int s0 = colptr[i], s1 = colptr[i + 1];
                if (!whole) {
                    s0 = rk_lower_bound(crow, s0, s1, lo);
                    s1 = rk_lower_bound(crow, s0, s1, lo + bn);
                }
                for (int p = s0 + lane; p < s1; p += 64) {
                    const int v = crow[p] - lo;
                    if ((unsigned)v < (unsigned)bn) atomicAdd(reinterpret_cast<int *>(acc) + v, q * (int)cval[p]);
                }
            }
            __syncthreads();
            if (tid == 0 && u >= lo && u < lo + bn) acc[u - lo] = 0;  // self: one more zero candidate
            __syncthreads();
            {
#pragma clang fp contract(off)
                for (int j = tid; j < bn; j += kKnnThreads) {
                    const int d = (int)acc[j];
                    if (d != 0) acc[j] = __float_as_uint(((float)d * ru) * rnorm[lo + j]);
                }
            }
            __syncthreads();
            floor_ = knn_fold(acc, bn, top, hist, misc, kk, floor_);
        }
        // descending bitonic sort of top[0, 128) (zeros beyond kk), 64 compare-exchanges per step
#pragma unroll 1
        for (int size = 2; size <= RK_KNN_MAX_K; size <<= 1) {
#pragma unroll 1
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (tid < RK_KNN_MAX_K / 2) {
                    const int pos = (tid / stride) * 2 * stride + (tid % stride), j = pos + stride;
                    const unsigned a = top[pos], b = top[j];
                    const bool desc = (pos & size) == 0;
                    if ((a < b) == desc && a != b) { top[pos] = b; top[j] = a; }
                }
                __syncthreads();
            }
        }
    } else {
        __syncthreads();
    }
    if (topw) for (int j = tid; j < k; j += kKnnThreads) topw[(size_t)u * k + j] = __uint_as_float(top[j]);
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < kk; ++j) s += (double)__uint_as_float(top[j]);
        degsim[u] = kk > 0 ? (float)(s / (double)kk) : 0.0f;
    }
}

RK_EXPORT int rk_knn_degsim(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                            const int32_t *colptr, const int32_t *crow, const float *cval, const float *rnorm, int32_t k, int32_t band,
                            const int32_t *order, float *topw, float *degsim, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || !rowptr || !col || !val || !colptr || !crow || !cval || !rnorm || !degsim)
        RK_FAIL(RK_EINVAL, "rk_knn_degsim: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_knn_degsim: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (band != 0 && (band < 64 || band > RK_KNN_MAX_BAND || band % 64))
        RK_FAIL(RK_EINVAL, "rk_knn_degsim: band = %d (0, or a multiple of 64 in 64..%d)", band, RK_KNN_MAX_BAND);
    if (band == 0) {
        const int n_bands = (n_users + kKnnAutoBand - 1) / kKnnAutoBand;
        band = (((n_users + n_bands - 1) / n_bands) + 63) / 64 * 64;
    }
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(knn_degsim_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsMaxBytes - 64));
        attr_once.done(attr_dev);
    }
    const size_t lds = (size_t)4 * band + kKnnScratchBytes;
    hipLaunchKernelGGL(knn_degsim_kernel, dim3(n_users), dim3(kKnnThreads), lds, (hipStream_t)stream, n_users, n_items, rowptr, col, val,
                       colptr, crow, cval, rnorm, k, band, order, topw, degsim);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_knn_select(int32_t n, const float *score, int32_t m, int32_t largest, int32_t *order_out, void *stream)
{
    return rk_select_ids("rk_knn_select", "scores", n, score, m, largest, order_out, stream);
}
