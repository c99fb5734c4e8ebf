// RP3beta victim: random-walk item-item scoring (Cooper et al. 2014; Christoffel et al. 2015; Paudel et al. 2017) from the
// U x I rating CSR and its transpose (rk_pca_transpose).  No I x I matrix is formed.  Every transition probability of the second
// step is carried as a 40-bit fixed-point integer (rk_rp3_steps), so the dots S_ij of rk_rp3_neighbors are sums of integers: one
// workgroup per item i walks the rows of the users of column i and adds P_uj of a band of candidate items j into 64-bit LDS
// accumulators with integer atomics (exact in any arrival order).  The weights are formed from S in double, rounded once to fp32,
// and selected with ItemKNN's key list (item_list.h).  rk_rp3_scores gives a wave a user: the wave walks the user's items in
// ascending order and scatters each item's kept list into an fp32 row of one column band in LDS; rk_rp3_pair_scores forms the
// same sum for explicit pairs, a wave per pair.  include/recad_hip.h states the definition.
#include <algorithm>
#include <math.h>

#include "common.h"
#include "item_list.h"

typedef unsigned long long rp_sum;

// LDS of one neighbour workgroup: the list scratch of item_list.h | rp_sum acc[band]
static_assert(8 * RK_RP3_MAX_BAND + kIkNbrScratchBytes <= kLdsMaxBytes - 64, "RK_RP3_MAX_BAND does not fit a CU's LDS");
static_assert(8 * (RK_RP3_MAX_BAND + 64) + kIkNbrScratchBytes > kLdsMaxBytes - 64, "RK_RP3_MAX_BAND is not the largest band");
static_assert(RK_RP3_MAX_BAND % 64 == 0 && kIkNbrScratchBytes % 16 == 0, "bands are multiples of 64, the accumulators 16-byte aligned");
static_assert(RK_RP3_MAX_USERS == (1 << 23), "n_i * 2^40 < 2^63 needs U < 2^23");
static constexpr int kRpAutoBand = 4096;                        // automatic fit band: 36 KiB per workgroup, 4 workgroups per CU
static constexpr int kRpAutoScoreBand = 8192;                   // automatic score band: a 32 KiB row per single-wave workgroup, 4 per CU
static constexpr double kRpScale = 1099511627776.0;             // 2^40
static constexpr double kRpUnscale = 1.0 / 1099511627776.0;     // 2^-40

static bool rp_exponent_ok(double e) { return e >= 0.0 && e <= 4.0; }       // false for NaN

// x^e; e == 1 and e == 0 are taken without pow, so those cases do not depend on the math library
__device__ __forceinline__ double rp_pow(double x, double e)
{
    if (e == 1.0) return x;
    if (e == 0.0) return 1.0;
    return pow(x, e);
}

// n^-e for a count n >= 1 (0 for n == 0): the IEEE quotient at e == 1, 1 at e == 0
__device__ __forceinline__ double rp_factor(int n, double e)
{
    if (n <= 0) return 0.0;
    if (e == 1.0) return 1.0 / (double)n;
    if (e == 0.0) return 1.0;
    return pow((double)n, -e);
}

// ---- steps: one wave per user
__global__ __launch_bounds__(256) void rp3_steps_kernel(int n_users, const int *__restrict__ rowptr, const float *__restrict__ val,
                                                        double alpha, long long *__restrict__ P, long long *__restrict__ r)
{
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const int beg = rowptr[u], end = rowptr[u + 1];
    long long s = 0;
    for (int e = beg + lane; e < end; e += 64) s += (long long)(int)val[e];
    s = wave_sum(s);
    if (lane == 0) r[u] = s;
    const double rd = (double)s;
    for (int e = beg + lane; e < end; e += 64) {
        const double p = rp_pow((double)(int)val[e] / rd, alpha);
        const long long x = (long long)rint(p * kRpScale);
        P[e] = x < 1 ? 1 : x;
    }
}

RK_EXPORT int rk_rp3_steps(int32_t n_users, const int32_t *rowptr, const float *val, double alpha, int64_t *P, int64_t *r, void *stream)
{
    if (n_users <= 0 || !rowptr || !val || !P || !r) RK_FAIL(RK_EINVAL, "rk_rp3_steps: bad arguments");
    if (n_users >= RK_RP3_MAX_USERS) RK_FAIL(RK_EINVAL, "rk_rp3_steps: %d users, fewer than %d keep every dot below 2^63", n_users, RK_RP3_MAX_USERS);
    if (!rp_exponent_ok(alpha)) RK_FAIL(RK_EINVAL, "rk_rp3_steps: alpha = %g outside [0, 4]", alpha);
    hipLaunchKernelGGL(rp3_steps_kernel, dim3((n_users + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_users, rowptr, val, alpha,
                       reinterpret_cast<long long *>(P), reinterpret_cast<long long *>(r));
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- factors
__global__ __launch_bounds__(256) void rp3_factors_kernel(int n_items, const int *__restrict__ colptr, double alpha, double beta,
                                                          double *__restrict__ fa, double *__restrict__ fb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int n = colptr[i + 1] - colptr[i];
    fa[i] = rp_factor(n, alpha);
    fb[i] = rp_factor(n, beta);
}

RK_EXPORT int rk_rp3_factors(int32_t n_items, const int32_t *colptr, double alpha, double beta, double *fa, double *fb, void *stream)
{
    if (n_items <= 0 || !colptr || !fa || !fb) RK_FAIL(RK_EINVAL, "rk_rp3_factors: bad arguments");
    if (!rp_exponent_ok(alpha)) RK_FAIL(RK_EINVAL, "rk_rp3_factors: alpha = %g outside [0, 4]", alpha);
    if (!rp_exponent_ok(beta)) RK_FAIL(RK_EINVAL, "rk_rp3_factors: beta = %g outside [0, 4]", beta);
    hipLaunchKernelGGL(rp3_factors_kernel, dim3((n_items + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_items, colptr, alpha, beta, fa, fb);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- neighbours: itemknn_neighbors_kernel with 64-bit accumulators fed from P, and the weight formed in double
__global__ __launch_bounds__(kIkThreads) void rp3_neighbors_kernel(int n_users, int n_items, const int *__restrict__ rowptr,
                                                                   const int *__restrict__ col, const rp_sum *__restrict__ P,
                                                                   const int *__restrict__ colptr, const int *__restrict__ crow,
                                                                   const double *__restrict__ fa, const double *__restrict__ fb, int k, int band,
                                                                   const int *__restrict__ order, int *__restrict__ nbr_id,
                                                                   float *__restrict__ nbr_w)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
    ik_key *buf = reinterpret_cast<ik_key *>(rp_lds);
    unsigned *misc = reinterpret_cast<unsigned *>(rp_lds + 8 * kIkKeys);
    rp_sum *acc = reinterpret_cast<rp_sum *>(rp_lds + kIkNbrScratchBytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = order ? order[blockIdx.x] : (int)blockIdx.x;
    if (i < 0 || i >= n_items) return;                                 // `order` is not a permutation: nothing is written for this entry
    const int kk = min(k, n_items - 1);
    for (int j = tid; j < kIkKeys; j += kIkThreads) buf[j] = 0;
    if (tid == 0) misc[0] = 0;
    const int beg = colptr[i], end = colptr[i + 1];
    const double fai = fa[i];
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
                int s0 = rowptr[u], s1 = rowptr[u + 1];
                if (!whole && s1 - s0 > kIkSearchFrom) {
                    s0 = rk_lower_bound(col, s0, s1, lo);
                    s1 = rk_lower_bound(col, s0, s1, lo + bn);
                }
                for (int p = s0 + lane; p < s1; p += 64) {
                    const int j = col[p] - lo;
                    if ((unsigned)j < (unsigned)bn) atomicAdd(acc + j, P[p]);
                }
            }
            __syncthreads();
            // candidates of this band, 256 at a time, as in itemknn_neighbors_kernel: a key above T joins the pending area; when
            // it would overflow, list and pending are sorted together, the first kk keys stay and T rises
#pragma unroll 1
            for (int c0 = 0; c0 < bn; c0 += kIkThreads) {
                const int j = c0 + tid;
                ik_key key = 0;
                if (j < bn && lo + j != i) {
                    const rp_sum s = acc[j];
                    if (s > 0) {
#pragma clang fp contract(off)
                        const float w = (float)((((double)s * fai) * fb[lo + j]) * kRpUnscale);
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

RK_EXPORT int rk_rp3_neighbors(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const int64_t *P,
                               const int32_t *colptr, const int32_t *crow, const double *fa, const double *fb, int32_t k, int32_t band,
                               const int32_t *order, int32_t *nbr_id, float *nbr_w, void *stream)
{
    if (n_users <= 0 || n_items <= 0 || !rowptr || !col || !P || !colptr || !crow || !fa || !fb || !nbr_id || !nbr_w)
        RK_FAIL(RK_EINVAL, "rk_rp3_neighbors: bad arguments");
    if (n_users >= RK_RP3_MAX_USERS)
        RK_FAIL(RK_EINVAL, "rk_rp3_neighbors: %d users, fewer than %d keep every dot below 2^63", n_users, RK_RP3_MAX_USERS);
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_rp3_neighbors: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (int rc = ik_resolve_band("rk_rp3_neighbors", &band, RK_RP3_MAX_BAND, kRpAutoBand, n_items)) return rc;
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rp3_neighbors_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kLdsMaxBytes - 64));
        attr_once.done(attr_dev);
    }
    const size_t lds = (size_t)8 * band + kIkNbrScratchBytes;
    hipLaunchKernelGGL(rp3_neighbors_kernel, dim3(n_items), dim3(kIkThreads), lds, (hipStream_t)stream, n_users, n_items, rowptr, col,
                       reinterpret_cast<const rp_sum *>(P), colptr, crow, fa, fb, k, band, order, nbr_id, nbr_w);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- scores
// One single-wave workgroup per entry of user_ids.  Per band of columns the fp32 row sits in LDS; the wave takes the user's items
// 64 at a time into its lanes and walks them in ascending order, the (at most 128) slots of an item's list across the lanes in
// two trips.  The ids of one list are distinct, so the lanes of one trip never meet; LDS operations of a wave complete in program
// order, which gives the ascending-i order of every column's sum.  The list of the next item is loaded while this one is added.
__global__ __launch_bounds__(64) void rp3_scores_kernel(int n_users, int n_items, int k, const int *__restrict__ nbr_id,
                                                        const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                        const int *__restrict__ col, const float *__restrict__ val,
                                                        const int *__restrict__ user_ids, int band, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float rp_row[];
    const int lane = threadIdx.x;
    const int u = user_ids[blockIdx.x];
    const bool known = u >= 0 && u < n_users;                          // an id out of range is a user with no items
    const int beg = known ? rowptr[u] : 0, end = known ? rowptr[u + 1] : 0;
    float *o = out + (size_t)blockIdx.x * n_items;
    const bool two = k > 64;
#pragma unroll 1
    for (int lo = 0; lo < n_items; lo += band) {
        const int bn = min(band, n_items - lo);
        for (int j = lane; j < bn; j += 64) rp_row[j] = 0.0f;
        __syncthreads();
        for (int c0 = beg; c0 < end; c0 += 64) {
            const int n = min(64, end - c0);
            int ci = -1;
            float qi = 0.0f;
            if (lane < n) {
                ci = col[c0 + lane];
                qi = (float)(int)val[c0 + lane];
                if ((unsigned)ci >= (unsigned)n_items) ci = -1;
            }
            int id0 = -1, id1 = -1;
            float w0 = 0.0f, w1 = 0.0f;
            int i = __shfl(ci, 0, 64);
            if (i >= 0) {
                if (lane < k) { id0 = nbr_id[(size_t)lane * n_items + i]; w0 = nbr_w[(size_t)lane * n_items + i]; }
                if (two && lane + 64 < k) { id1 = nbr_id[(size_t)(lane + 64) * n_items + i]; w1 = nbr_w[(size_t)(lane + 64) * n_items + i]; }
            }
            for (int x = 0; x < n; ++x) {
                const float q = __shfl(qi, x, 64);
                const int a0 = id0 - lo, a1 = id1 - lo;
                const float v0 = w0, v1 = w1;
                id0 = id1 = -1;
                if (x + 1 < n) {
                    i = __shfl(ci, x + 1, 64);
                    if (i >= 0) {
                        if (lane < k) { id0 = nbr_id[(size_t)lane * n_items + i]; w0 = nbr_w[(size_t)lane * n_items + i]; }
                        if (two && lane + 64 < k) { id1 = nbr_id[(size_t)(lane + 64) * n_items + i]; w1 = nbr_w[(size_t)(lane + 64) * n_items + i]; }
                    }
                }
                // id - lo of an unused slot (-1) is negative: outside the band like any other column of another band
                if ((unsigned)a0 < (unsigned)bn) rp_row[a0] = ik_add_term(rp_row[a0], v0, q);
                if ((unsigned)a1 < (unsigned)bn) rp_row[a1] = ik_add_term(rp_row[a1], v1, q);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        for (int j = lane; j < bn; j += 64) o[lo + j] = rp_row[j];
        __syncthreads();
    }
}

RK_EXPORT int rk_rp3_scores(int32_t n_users, int32_t n_items, int32_t k, const int32_t *nbr_id, const float *nbr_w, const int32_t *rowptr,
                            const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids, int32_t band, float *out,
                            void *stream)
{
    if (n_users <= 0 || n_items <= 0 || nb < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val || !user_ids || !out)
        RK_FAIL(RK_EINVAL, "rk_rp3_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_rp3_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (int rc = ik_resolve_band("rk_rp3_scores", &band, RK_RP3_MAX_BAND, kRpAutoScoreBand, n_items)) return rc;
    if (nb == 0) return RK_OK;                                         // after the refusal of a bad band, as before
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rp3_scores_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   4 * RK_RP3_MAX_BAND));
        attr_once.done(attr_dev);
    }
    hipLaunchKernelGGL(rp3_scores_kernel, dim3(nb), dim3(64), (size_t)4 * band, (hipStream_t)stream, n_users, n_items, k, nbr_id, nbr_w,
                       rowptr, col, val, user_ids, band, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---- pairs: one wave per (user, item j).  The user's items in ascending order; the lanes look for j in the slots of item i's
// list (at most one holds it), the weight found is handed to every lane and added as the matrix kernel adds it.
__global__ __launch_bounds__(256) void rp3_pair_kernel(int n_items, int n_users, int k, const int *__restrict__ nbr_id,
                                                       const float *__restrict__ nbr_w, const int *__restrict__ rowptr,
                                                       const int *__restrict__ col, const float *__restrict__ val,
                                                       const long long *__restrict__ users, const long long *__restrict__ items,
                                                       long long n, float *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    const long long u = users[p], jj = items[p];
    float s = 0.0f;
    if (u >= 0 && u < n_users && jj >= 0 && jj < n_items) {
        const int j = (int)jj;
        const int beg = rowptr[u], end = rowptr[u + 1];
        for (int c0 = beg; c0 < end; c0 += 64) {
            const int n_here = min(64, end - c0);
            int ci = -1;
            float qi = 0.0f;
            if (lane < n_here) {
                ci = col[c0 + lane];
                qi = (float)(int)val[c0 + lane];
                if ((unsigned)ci >= (unsigned)n_items) ci = -1;
            }
            for (int x = 0; x < n_here; ++x) {
                const int i = __shfl(ci, x, 64);
                const float q = __shfl(qi, x, 64);
                if (i < 0) continue;
                float w = 0.0f;
                bool hit = false;
                for (int t = lane; t < k; t += 64)
                    if (nbr_id[(size_t)t * n_items + i] == j) { w = nbr_w[(size_t)t * n_items + i]; hit = true; }
                const unsigned long long m = __ballot(hit);
                if (m) s = ik_add_term(s, __shfl(w, __ffsll((long long)m) - 1, 64), q);
            }
        }
    }
    if (lane == 0) out[p] = s;
}

RK_EXPORT int rk_rp3_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                                 const int32_t *rowptr, const int32_t *col, const float *val, const int64_t *users, const int64_t *items,
                                 int64_t n, float *out, void *stream)
{
    if (n_items <= 0 || n_users <= 0 || n < 0 || !nbr_id || !nbr_w || !rowptr || !col || !val) RK_FAIL(RK_EINVAL, "rk_rp3_pair_scores: bad arguments");
    if (k < 1 || k > RK_KNN_MAX_K) RK_FAIL(RK_EINVAL, "rk_rp3_pair_scores: k = %d outside 1..%d", k, RK_KNN_MAX_K);
    if (n == 0) return RK_OK;
    if (!users || !items || !out) RK_FAIL(RK_EINVAL, "rk_rp3_pair_scores: bad arguments");
    if ((n + 3) / 4 > 0x7fffffffLL) RK_FAIL(RK_EINVAL, "rk_rp3_pair_scores: too many pairs");
    hipLaunchKernelGGL(rp3_pair_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n_items, n_users, k, nbr_id, nbr_w,
                       rowptr, col, val, reinterpret_cast<const long long *>(users), reinterpret_cast<const long long *>(items),
                       (long long)n, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
