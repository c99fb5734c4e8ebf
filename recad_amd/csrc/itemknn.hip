// ItemKNN victim: item-neighbourhood scoring (Sarwar et al. 2001; Deshpande and Karypis 2004) from the U x I rating CSR and
// its transpose (rk_pca_transpose).  No I x I matrix is formed.  rk_itemknn_neighbors is knn_degsim_kernel with the two
// orientations swapped: one workgroup per item i walks the rows of the users of column i and accumulates the integer dots d_ij
// of a band of candidate items in LDS (integer adds: exact in any arrival order).  Unlike DegSim the list carries IDS, so the
// selection orders 64-bit keys (bits of w) << 32 | (0xFFFFFFFF - j): all distinct, descending key = (w descending, j
// ascending), and an unordered gather followed by a sort is deterministic.  rk_itemknn_scores stages a block of users' rows in
// LDS as dense byte rows and sums the table's slots in order; rk_itemknn_pair_scores forms the same sum for explicit pairs.
// include/recad_hip.h states the definition.
#include <algorithm>

#include "common.h"
#include "item_list.h"   // the key list, its sort and the band constants, shared with rp3beta.hip

static_assert(4 * RK_ITEMKNN_MAX_BAND + kIkNbrScratchBytes <= kLdsMaxBytes - 64, "RK_ITEMKNN_MAX_BAND does not fit a CU's LDS");
static_assert(4 * (RK_ITEMKNN_MAX_BAND + 64) + kIkNbrScratchBytes > kLdsMaxBytes - 64, "RK_ITEMKNN_MAX_BAND is not the largest band");
static_assert(RK_ITEMKNN_MAX_BAND % 64 == 0, "bands are multiples of 64");
static constexpr int kIkAutoBand = 8192;                        // automatic band: 36 KiB per workgroup, 4 workgroups per CU
// the scoring kernel's LDS holds byte rows only (no scratch), each padded to 16 bytes
static constexpr int kIkScoreLdsBytes = kLdsMaxBytes - 64;
static_assert(RK_ITEMKNN_MAX_ITEMS % 16 == 0 && RK_ITEMKNN_MAX_ITEMS <= kIkScoreLdsBytes && RK_ITEMKNN_MAX_ITEMS + 16 > kIkScoreLdsBytes,
              "RK_ITEMKNN_MAX_ITEMS is the largest catalogue whose single byte row fits a CU's LDS");
static_assert(RK_ITEMKNN_MAX_USER_BLOCK == 16, "the scoring kernel is instantiated for 1, 2, 4, 8 and 16 accumulators");

__global__ __launch_bounds__(kIkThreads) void itemknn_neighbors_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                                       const int *__restrict__ col, const float *__restrict__ val,
                                                                       const int *__restrict__ colptr, const int *__restrict__ crow,
                                                                       const float *__restrict__ cval, const float *__restrict__ rnorm_item,
                                                                       int k, int band, const int *__restrict__ order,
                                                                       int *__restrict__ nbr_id, float *__restrict__ nbr_w)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ik_lds[];
    ik_key *buf = reinterpret_cast<ik_key *>(ik_lds);
    unsigned *misc = reinterpret_cast<unsigned *>(ik_lds + 8 * kIkKeys);
    int *acc = reinterpret_cast<int *>(ik_lds + kIkNbrScratchBytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = order ? order[blockIdx.x] : (int)blockIdx.x;
    if (i < 0 || i >= n_items) return;                                 // `order` is not a permutation: nothing is written for this entry
    const int kk = min(k, n_items - 1);
    for (int j = tid; j < kIkKeys; j += kIkThreads) buf[j] = 0;
    if (tid == 0) misc[0] = 0;
    const int beg = colptr[i], end = colptr[i + 1];
    const float ri = rnorm_item[i];
    ik_key T = 0;                                                      // the kk-th key of the list once it is full: smaller keys can never enter
    int n_pend = 0, phase = 0;
    __syncthreads();
    if (kk > 0 && end > beg) {
#pragma unroll 1
        for (int lo = 0; lo < n_items; lo += band) {
            const int bn = min(band, n_items - lo);
            for (int j = tid; j < bn; j += kIkThreads) acc[j] = 0;
            __syncthreads();
            const bool whole = lo == 0 && bn == n_items;
            for (int e = beg + wave; e < end; e += kIkThreads / 64) {
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
            // candidates of this band, 256 at a time: a key above T joins the pending area; when it would overflow, list and
            // pending are sorted together, the first kk keys stay and T rises
#pragma unroll 1
            for (int c0 = 0; c0 < bn; c0 += kIkThreads) {
                const int j = c0 + tid;
                ik_key key = 0;
                if (j < bn && lo + j != i) {
                    const int d = acc[j];
                    if (d > 0) {
#pragma clang fp contract(off)
                        const float w = ((float)d * ri) * rnorm_item[lo + j];
                        key = ((ik_key)__float_as_uint(w) << 32) | (ik_key)(0xFFFFFFFFu - (unsigned)(lo + j));
                    }
                }
                bool pass = key > T;
                int cnt = ik_block_count(pass, misc + 4, phase);
                if (cnt == 0) continue;
                if (n_pend + cnt > kIkPending) {
                    ik_sort(buf);
                    for (int t = kk + tid; t < kIkKeys; t += kIkThreads) buf[t] = 0;
                    if (tid == 0) misc[0] = 0;
                    T = buf[kk - 1];
                    n_pend = 0;
                    pass = key > T;
                    cnt = ik_block_count(pass, misc + 4, phase);
                }
                if (pass) {
                    const unsigned pos = atomicAdd(&misc[0], 1u);
                    if (pos < (unsigned)kIkPending) buf[RK_KNN_MAX_K + pos] = key;
                }
                n_pend += cnt;
            }
            __syncthreads();
        }
        ik_sort(buf);
    }
    for (int t = tid; t < k; t += kIkThreads) {
        const ik_key key = t < kk ? buf[t] : 0;
        nbr_id[(size_t)t * n_items + i] = key ? (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu)) : -1;
        nbr_w[(size_t)t * n_items + i] = __uint_as_float((unsigned)(key >> 32));
    }
}

RK_EXPORT int rk_itemknn_neighbors(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                                   const int32_t *colptr, const int32_t *crow, const float *cval, const float *rnorm_item, int32_t k,
                                   int32_t band, const int32_t *order, int32_t *nbr_id, float *nbr_w, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || !rowptr || !col || !val || !colptr || !crow || !cval || !rnorm_item || !nbr_id || !nbr_w)
        RK_FAIL(RK_EINVAL, "rk_itemknn_neighbors: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_itemknn_neighbors: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (int rc = ik_resolve_band("rk_itemknn_neighbors", &band, RK_ITEMKNN_MAX_BAND, kIkAutoBand, n_items)) return rc;
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_neighbors_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsMaxBytes - 64));
        attr_once.done(attr_dev);
    }
    const size_t lds = (size_t)4 * band + kIkNbrScratchBytes;
    hipLaunchKernelGGL(itemknn_neighbors_kernel, dim3(n_items), dim3(kIkThreads), lds, (hipStream_t)stream, n_users, n_items, rowptr, col,
                       val, colptr, crow, cval, rnorm_item, k, band, order, nbr_id, nbr_w);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- scores
// Block x of the grid stages users [x * ub, x * ub + ub) of user_ids as byte rows; block y walks items [y * seg, y * seg + seg).
// A lane owns an item: slot t of 64 consecutive items is one coalesced line of each table, read once for the ub users.
template <int UB>
__global__ __launch_bounds__(kIkThreads) void itemknn_scores_kernel(int n_items, int k, const int *__restrict__ nbr_id,
                                                                    const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                                    const int *__restrict__ col, const float *__restrict__ val, int nb,
                                                                    const int *__restrict__ user_ids, int ub, int row_bytes, int seg,
                                                                    float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ik_rows[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * ub, n_rows = min(ub, nb - b0);
    uint4 *z = reinterpret_cast<uint4 *>(ik_rows);
    for (int j = tid; j < ub * (row_bytes / 16); j += kIkThreads) z[j] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int b = wave; b < n_rows; b += kIkThreads / 64) {
        const int u = user_ids[b0 + b];
        const int beg = rowptr[u], end = rowptr[u + 1];
        for (int e = beg + lane; e < end; e += 64) {
            const int c = col[e];
            if ((unsigned)c < (unsigned)n_items) ik_rows[(size_t)b * row_bytes + c] = (unsigned char)(int)val[e];
        }
    }
    __syncthreads();
    const int i1 = min(n_items, ((int)blockIdx.y + 1) * seg);
    for (int i = blockIdx.y * seg + tid; i < i1; i += kIkThreads) {
        float s[UB];
#pragma unroll
        for (int b = 0; b < UB; ++b) s[b] = 0.0f;
        for (int t = 0; t < k; ++t) {
            const int id = nbr_id[(size_t)t * n_items + i];
            const float w = nbr_w[(size_t)t * n_items + i];
            if ((unsigned)id >= (unsigned)n_items) continue;          // an unused slot (-1) adds nothing
#pragma unroll
            for (int b = 0; b < UB; ++b)
                if (b < ub) s[b] = ik_add_term(s[b], w, (float)ik_rows[(size_t)b * row_bytes + id]);
        }
#pragma unroll
        for (int b = 0; b < UB; ++b)
            if (b < n_rows) out[(size_t)(b0 + b) * n_items + i] = s[b];
    }
}

RK_EXPORT int rk_itemknn_scores(int32_t n_items, int32_t k, const int32_t *nbr_id, const float *nbr_w, const int32_t *rowptr,
                                const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids, int32_t user_block, float *out,
                                void *stream)
{
    if (n_items <= 0 || nb < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val || !user_ids || !out)
        RK_FAIL(RK_EINVAL, "rk_itemknn_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_itemknn_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (n_items > RK_ITEMKNN_MAX_ITEMS)
        RK_FAIL(RK_EINVAL, "rk_itemknn_scores: %d items, one byte row of at most %d fits a CU's LDS", n_items, RK_ITEMKNN_MAX_ITEMS);
    const int row_bytes = (n_items + 15) / 16 * 16, fit = kIkScoreLdsBytes / row_bytes;
    if (user_block < 0 || user_block > RK_ITEMKNN_MAX_USER_BLOCK)
        RK_FAIL(RK_EINVAL, "rk_itemknn_scores: user_block = %d (0, or 1..%d)", user_block, RK_ITEMKNN_MAX_USER_BLOCK);
    if (user_block > fit)
        RK_FAIL(RK_EINVAL, "rk_itemknn_scores: user_block = %d, only %d byte rows of %d items fit a CU's LDS", user_block, fit, n_items);
    if (nb == 0) return RK_OK;
    int ub = user_block ? user_block : std::min((int)RK_ITEMKNN_MAX_USER_BLOCK, fit);
    ub = std::min(ub, (int)nb);
    const int n_blocks = (nb + ub - 1) / ub;
    // enough workgroups to fill the chip: the item range is split when the user blocks alone are few
    const int max_y = (n_items + kIkThreads - 1) / kIkThreads;
    const int want_y = std::max(1, std::min(max_y, 1024 / n_blocks));
    const int seg = ((n_items + want_y - 1) / want_y + kIkThreads - 1) / kIkThreads * kIkThreads;
    const int ny = (n_items + seg - 1) / seg;
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_scores_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kIkScoreLdsBytes));
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_scores_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, kIkScoreLdsBytes));
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_scores_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kIkScoreLdsBytes));
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_scores_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, kIkScoreLdsBytes));
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(itemknn_scores_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, kIkScoreLdsBytes));
        attr_once.done(attr_dev);
    }
    const size_t lds = (size_t)ub * row_bytes;
    const dim3 grid(n_blocks, ny), block(kIkThreads);
    hipStream_t s = (hipStream_t)stream;
#define IK_LAUNCH(UB) \
    hipLaunchKernelGGL(itemknn_scores_kernel<UB>, grid, block, lds, s, n_items, k, nbr_id, nbr_w, rowptr, col, val, nb, user_ids, ub, row_bytes, seg, out)
    if (ub == 1) IK_LAUNCH(1);
    else if (ub == 2) IK_LAUNCH(2);
    else if (ub <= 4) IK_LAUNCH(4);
    else if (ub <= 8) IK_LAUNCH(8);
    else IK_LAUNCH(16);
#undef IK_LAUNCH
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- pairs: one thread per (user, item); the item's slots in order, each neighbour looked up in the user's ascending row
__global__ __launch_bounds__(256) void itemknn_pair_kernel(int n_items, int n_users, int k, const int *__restrict__ nbr_id,
                                                           const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                           const int *__restrict__ col, const float *__restrict__ val,
                                                           const long long *__restrict__ users, const long long *__restrict__ items,
                                                           long long n, float *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long u = users[p], i = items[p];
    float s = 0.0f;
    if (u >= 0 && u < n_users && i >= 0 && i < n_items) {
        const int beg = rowptr[u], end = rowptr[u + 1];
        for (int t = 0; t < k; ++t) {
            const int id = nbr_id[(size_t)t * n_items + i];
            if ((unsigned)id >= (unsigned)n_items) continue;
            const int e = rk_find_sorted(col, beg, end, id);
            if (e >= 0) s = ik_add_term(s, nbr_w[(size_t)t * n_items + i], (float)(int)val[e]);
        }
    }
    out[p] = s;
}

RK_EXPORT int rk_itemknn_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                                     const int32_t *rowptr, const int32_t *col, const float *val, const int64_t *users,
                                     const int64_t *items, int64_t n, float *out, void *stream)
{
    if (n_items <= 0 || n_users <= 0 || n < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val) RK_FAIL(RK_EINVAL, "rk_itemknn_pair_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_itemknn_pair_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (n == 0) return RK_OK;
    if (!users || !items || !out) RK_FAIL(RK_EINVAL, "rk_itemknn_pair_scores: bad arguments");
    if ((n + 255) / 256 > 0x7fffffffLL) RK_FAIL(RK_EINVAL, "rk_itemknn_pair_scores: too many pairs");
    hipLaunchKernelGGL(itemknn_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_items, n_users, k, nbr_id,
                       nbr_w, rowptr, col, val, reinterpret_cast<const long long *>(users), reinterpret_cast<const long long *>(items),
                       (long long)n, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
