// UserKNN victim: user-neighbourhood scoring (Resnick et al. 1994; Breese et al. 1998; Herlocker et al. 1999), the recommender
// the average, segment and bandwagon profiles were designed against (Lam and Riedl 2004).  The neighbour tables are the work of
// rk_itemknn_neighbors on the transposed roles (itemknn.hip; include/recad_hip.h says how it is called), so this file holds the
// scoring alone.  rk_userknn_scores gives a wave a user: the wave takes the user's k neighbour ids and weights into its lanes
// once, walks the slots in ascending order and scatters each neighbour's whole rating row into an fp32 row of one column band in
// LDS (and, when normalising, the weight into a second row); rk_userknn_pair_scores forms the same sums for explicit pairs.
// include/recad_hip.h states the definition.
#include "common.h"
#include "item_list.h"   // ik_add_term, ik_resolve_band, kIkSearchFrom

// LDS of one scoring workgroup when normalising: float num[band] | float den[band]
static_assert(8 * RK_USERKNN_MAX_BAND <= kLdsMaxBytes - 64, "RK_USERKNN_MAX_BAND does not fit a CU's LDS");
static_assert(RK_USERKNN_MAX_BAND % 64 == 0, "bands are multiples of 64");
static constexpr int kUkAhead = 8;                              // slots whose first chunks are in flight together
static constexpr int kUkAutoBand = 8192;                        // automatic band: 32 or 64 KiB per single-wave workgroup, 5 or 2 per CU

// the segment [s0, s1) of neighbour row [beg, end) that can hold columns of [lo, lo + bn): a long row is searched, a short one
// is taken whole and filtered by the adds
__device__ __forceinline__ void uk_segment(const int *__restrict__ col, int beg, int end, bool whole, int lo, int bn, int &s0, int &s1)
{
    s0 = beg;
    s1 = end;
    if (!whole && end - beg > kIkSearchFrom) {
        s0 = rk_lower_bound(col, beg, end, lo);
        s1 = rk_lower_bound(col, s0, end, lo + bn);
    }
}

// ---- scores
// One single-wave workgroup per entry of user_ids.  Lane t holds slots t and t + 64 of the user's list: the id (an unused or
// foreign one becomes an empty row), the weight and the neighbour's row bounds, read once for all bands.  Per band the wave walks
// the slots in ascending order and spreads each neighbour's row over its lanes 64 entries at a time.  The columns of one row are
// distinct, so the lanes of one trip never meet; LDS operations of a wave complete in program order, which gives the slot order
// of every column's sum.  The first 64 entries of eight neighbours' rows are loaded together, ahead of their adds.
template <bool NORM>
__global__ __launch_bounds__(64) void userknn_scores_kernel(int n_users, int n_items, int k, const int *__restrict__ nbr_id,
                                                            const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                            const int *__restrict__ col, const float *__restrict__ val,
                                                            const int *__restrict__ user_ids, int band, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float uk_row[];
    float *num = uk_row, *den = uk_row + band;                         // den is touched only when NORM
    const int lane = threadIdx.x;
    const int u = user_ids[blockIdx.x];
    const bool known = u >= 0 && u < n_users;                          // an id out of range is a user with no neighbours
    float *o = out + (size_t)blockIdx.x * n_items;
    float w0 = 0.0f, w1 = 0.0f;
    int b0 = 0, e0 = 0, b1 = 0, e1 = 0;
    if (known && lane < k) {
        const int v = nbr_id[(size_t)lane * n_users + u];
        if ((unsigned)v < (unsigned)n_users) { w0 = nbr_w[(size_t)lane * n_users + u]; b0 = rowptr[v]; e0 = rowptr[v + 1]; }
    }
    if (known && lane + 64 < k) {
        const int v = nbr_id[(size_t)(lane + 64) * n_users + u];
        if ((unsigned)v < (unsigned)n_users) { w1 = nbr_w[(size_t)(lane + 64) * n_users + u]; b1 = rowptr[v]; e1 = rowptr[v + 1]; }
    }
    const int kk = known ? k : 0;
#pragma unroll 1
    for (int lo = 0; lo < n_items; lo += band) {
        const int bn = min(band, n_items - lo);
        for (int j = lane; j < bn; j += 64) {
            num[j] = 0.0f;
            if (NORM) den[j] = 0.0f;
        }
        __syncthreads();
        const bool whole = lo == 0 && bn == n_items;
        // the slots kUkAhead at a time: their segments and first chunks first, so that the loads are in flight together, then
        // their adds one slot after the other
#pragma unroll 1
        for (int t0 = 0; t0 < kk; t0 += kUkAhead) {
            int s0[kUkAhead], s1[kUkAhead], rc[kUkAhead];
            float w[kUkAhead], rv[kUkAhead];
            // every load is issued whether or not the lane has an entry (the address falls back to entry 0, which exists), and
            // nothing uses a loaded value before the second loop: a use next to its load would make the wave wait there
#pragma unroll
            for (int x = 0; x < kUkAhead; ++x) {
                const int t = t0 + x;
                const bool hi = t >= 64;
                // one slot's bounds for the whole wave: said so, the segment search runs on scalars
                const int beg = __builtin_amdgcn_readfirstlane(__shfl(hi ? b1 : b0, t & 63, 64));
                const int end = __builtin_amdgcn_readfirstlane(__shfl(hi ? e1 : e0, t & 63, 64));
                w[x] = __shfl(hi ? w1 : w0, t & 63, 64);
                uk_segment(col, t < kk ? beg : 0, t < kk ? end : 0, whole, lo, bn, s0[x], s1[x]);
                const int p = s0[x] + lane < s1[x] ? s0[x] + lane : 0;
                rc[x] = col[p];
                rv[x] = val[p];
            }
#pragma unroll
            for (int x = 0; x < kUkAhead; ++x) {
                // a lane without an entry, or a column of another band, is outside [0, bn)
                const int cj = s0[x] + lane < s1[x] ? rc[x] - lo : -1;
                if ((unsigned)cj < (unsigned)bn) {
                    num[cj] = ik_add_term(num[cj], w[x], (float)(int)rv[x]);
                    if (NORM) den[cj] = den[cj] + w[x];
                }
                for (int p = s0[x] + 64 + lane; p < s1[x]; p += 64) {
                    const int j = col[p] - lo;
                    if ((unsigned)j < (unsigned)bn) {
                        num[j] = ik_add_term(num[j], w[x], (float)(int)val[p]);
                        if (NORM) den[j] = den[j] + w[x];
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        for (int j = lane; j < bn; j += 64) {
            float s = num[j];
            if (NORM) {
                const float d = den[j];
                s = d > 0.0f ? __fdiv_rn(s, d) : 0.0f;
            }
            o[lo + j] = s;
        }
        __syncthreads();
    }
}

RK_EXPORT int rk_userknn_scores(int32_t n_users, int32_t n_items, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                                const int32_t *rowptr, const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids,
                                int32_t normalize, int32_t band, float *out, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || nb < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val || !user_ids || !out)
        RK_FAIL(RK_EINVAL, "rk_userknn_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_userknn_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (normalize != 0 && normalize != 1) RK_FAIL(RK_EINVAL, "rk_userknn_scores: normalize = %d (0 or 1)", normalize);
    if (int rc = ik_resolve_band("rk_userknn_scores", &band, RK_USERKNN_MAX_BAND, kUkAutoBand, n_items)) return rc;
    if (nb == 0) return RK_OK;
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(userknn_scores_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   4 * RK_USERKNN_MAX_BAND));
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(userknn_scores_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   8 * RK_USERKNN_MAX_BAND));
        attr_once.done(attr_dev);
    }
    if (normalize)
        hipLaunchKernelGGL(userknn_scores_kernel<true>, dim3(nb), dim3(64), (size_t)8 * band, (hipStream_t)stream, n_users, n_items, k, nbr_id,
                           nbr_w, rowptr, col, val, user_ids, band, out);
    else
        hipLaunchKernelGGL(userknn_scores_kernel<false>, dim3(nb), dim3(64), (size_t)4 * band, (hipStream_t)stream, n_users, n_items, k, nbr_id,
                           nbr_w, rowptr, col, val, user_ids, band, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- pairs: one thread per (user, item j); the user's slots in order, j looked up in each neighbour's ascending row
__global__ __launch_bounds__(256) void userknn_pair_kernel(int n_items, int n_users, int k, const int *__restrict__ nbr_id,
                                                           const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                           const int *__restrict__ col, const float *__restrict__ val,
                                                           const long long *__restrict__ users, const long long *__restrict__ items,
                                                           long long n, int normalize, float *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long u = users[p], j = items[p];
    float s = 0.0f, d = 0.0f;
    if (u >= 0 && u < n_users && j >= 0 && j < n_items) {
        for (int t = 0; t < k; ++t) {
            const int v = nbr_id[(size_t)t * n_users + u];
            if ((unsigned)v >= (unsigned)n_users) continue;
            const int e = rk_find_sorted(col, rowptr[v], rowptr[v + 1], (int)j);
            if (e < 0) continue;
            const float w = nbr_w[(size_t)t * n_users + u];
            s = ik_add_term(s, w, (float)(int)val[e]);
            d = d + w;
        }
    }
    if (normalize) s = d > 0.0f ? __fdiv_rn(s, d) : 0.0f;
    out[p] = s;
}

RK_EXPORT int rk_userknn_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                                     const int32_t *rowptr, const int32_t *col, const float *val, const int64_t *users,
                                     const int64_t *items, int64_t n, int32_t normalize, float *out, void *stream)
{
    if (n_items <= 0 || n_users <= 0 || n < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val) RK_FAIL(RK_EINVAL, "rk_userknn_pair_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_userknn_pair_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (normalize != 0 && normalize != 1) RK_FAIL(RK_EINVAL, "rk_userknn_pair_scores: normalize = %d (0 or 1)", normalize);
    if (n == 0) return RK_OK;
    if (!users || !items || !out) RK_FAIL(RK_EINVAL, "rk_userknn_pair_scores: bad arguments");
    if ((n + 255) / 256 > 0x7fffffffLL) RK_FAIL(RK_EINVAL, "rk_userknn_pair_scores: too many pairs");
    hipLaunchKernelGGL(userknn_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_items, n_users, k, nbr_id,
                       nbr_w, rowptr, col, val, reinterpret_cast<const long long *>(users), reinterpret_cast<const long long *>(items),
                       (long long)n, normalize, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
