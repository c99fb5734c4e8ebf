// FraudarSelectUsers defender: greedy peeling of the bipartite rating graph towards its densest block (Hooi, Song, Beutel, Shah,
// Shin, Faloutsos, "FRAUDAR: Bounding Graph Fraud in the Face of Camouflage", KDD 2016), in integers end to end: column weights
// in 24-bit fixed point from a host table, priorities and the block score in uint64, the best-block comparison as an exact
// 128-bit product.  include/recad_hip.h states the definition.
//
// The peel is one sequential chain of N = U + I removals, so one workgroup runs it (as rk_slim_fit runs a column): no grid
// barrier, no waiting on another workgroup, every loop bounded by its inputs.  pri stays in global memory (L2-resident); over
// it sits a hierarchy of (pri, id) minima in LDS: level 0 has one entry per leaf block of 64 nodes, level l one entry per 64
// entries of level l - 1, up to a single root.  One step: the root names v; the workgroup strides v's row (a user) or column (an
// item), each lane a plain read-modify-write of one distinct neighbour's pri, and flags the neighbour's leaf block; the flagged
// blocks of each level are reduced again, one wave per block, with a workgroup barrier between the levels.  The flags are bits
// set with LDS atomics, the first setter appends the block to the level's list: the list's order varies, the minima do not.
#include <limits.h>

#include "common.h"

static constexpr int kFdThreads = 1024;                        // 16 waves: the flagged blocks of a step are reduced side by side
static constexpr int kFdWaves = kFdThreads / 64;
static constexpr int kFdMaxLevels = 4;                         // 64^4 leaves: more than RK_FD_MAX_NODES
static constexpr unsigned long long kFdRemoved = ~0ULL;        // pri of a removed node
static constexpr int kFdBatch = 4;                             // leaf blocks whose loads a wave has in flight together
static constexpr int kFdTailBytes = 2 * kFdMaxLevels * 4 + kFdWaves * 8;   // two parities of list lengths, the f partials

struct FdShape {
    int levels;
    int nb[kFdMaxLevels];      // entries of level l
    int off[kFdMaxLevels];     // where level l starts in the entry arrays
    int total;                 // entries of all levels
};

__host__ __device__ inline FdShape fd_shape(int n_nodes)
{
    FdShape s;
    s.levels = 0;
    s.total = 0;
    int n = n_nodes;
    bool done = false;
#pragma unroll
    for (int l = 0; l < kFdMaxLevels; ++l) {                     // constant indices: the shape stays in registers
        s.nb[l] = s.off[l] = 0;
        if (!done) {
            n = (n + 63) / 64;
            s.nb[l] = n;
            s.off[l] = s.total;
            s.total += n;
            s.levels = l + 1;
            done = n <= 1;
        }
    }
    return s;
}

// per entry: pri 8, id 4, list 4; one flag bit; the tail
static inline size_t fd_lds_bytes(int total) { return (size_t)16 * total + 4 * (size_t)((total + 31) / 32) + kFdTailBytes; }

static constexpr long long fd_entries_of(long long n)
{
    long long total = 0;
    do {
        n = (n + 63) / 64;
        total += n;
    } while (n > 1);
    return total;
}
static constexpr long long fd_bytes_of(long long n) { return 16 * fd_entries_of(n) + 4 * ((fd_entries_of(n) + 31) / 32) + kFdTailBytes; }
static_assert(fd_bytes_of(RK_FD_MAX_NODES) <= kLdsMaxBytes - 64, "RK_FD_MAX_NODES does not fit a CU's LDS");
static_assert(fd_bytes_of(2LL * RK_FD_MAX_NODES) > kLdsMaxBytes - 64, "RK_FD_MAX_NODES is not the largest power of two that fits");
static_assert(RK_FD_MAX_NODES >= (1 << 17) && RK_FD_MAX_NODES <= 64LL * 64 * 64 * 64, "RK_FD_MAX_NODES against the hierarchy's depth");

// ---------------------------------------------------------------------------------------------------------------- rk_fd_init
// bad[0] <- the lowest item whose column length is outside 0..U; bad[1] <- the lowest degree met whose weight is outside 1..2^24
__global__ __launch_bounds__(256) void fd_check_kernel(int n_users, int n_items, const int *__restrict__ colptr, const unsigned *__restrict__ wtab,
                                                       unsigned long long *__restrict__ bad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int d = colptr[i + 1] - colptr[i];
    if (d < 0 || d > n_users) {
        atomicMin(&bad[0], (unsigned long long)i);
        return;
    }
    const unsigned w = wtab[d];
    if (w < 1u || w > RK_FD_WEIGHT_ONE) atomicMin(&bad[1], (unsigned long long)d);
}

// not rk_first_bad_status_kernel: two words, one per rule, and the degree rule goes first whatever the indices
__global__ void fd_status_kernel(const unsigned long long *__restrict__ bad, int *__restrict__ status)
{
    const bool deg = bad[0] != ~0ULL, wt = bad[1] != ~0ULL;
    status[0] = deg ? RK_FD_BAD_DEGREE : (wt ? RK_FD_BAD_WEIGHT : 0);
    status[1] = deg ? (int)bad[0] : (wt ? (int)bad[1] : -1);
}

__global__ __launch_bounds__(256) void fd_item_kernel(int n_users, int n_items, const int *__restrict__ colptr, const unsigned *__restrict__ wtab,
                                                      unsigned *__restrict__ w_item, unsigned long long *__restrict__ pri)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const int d = colptr[i + 1] - colptr[i];
    const unsigned w = wtab[d];                                     // fd_check_kernel has seen 0 <= d <= U
    w_item[i] = w;
    pri[(size_t)n_users + i] = (unsigned long long)w * (unsigned long long)d;
}

// one wave per user
__global__ __launch_bounds__(256) void fd_user_kernel(int n_users, int n_items, long long nnz, const int *__restrict__ rowptr,
                                                      const int *__restrict__ col, const unsigned *__restrict__ w_item,
                                                      unsigned long long *__restrict__ pri)
{
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= n_users) return;
    const long long beg = max((long long)rowptr[u], 0LL), end = min((long long)rowptr[u + 1], nnz);
    unsigned long long s = 0;
    for (long long e = beg + lane; e < end; e += 64) {
        const int i = col[e];
        if ((unsigned)i < (unsigned)n_items) s += w_item[i];
    }
    s = wave_sum(s);
    if (lane == 0) pri[u] = s;
}

// f_0 = the sum of the items' priorities (every edge once, at its item's weight) = the sum of the users' priorities
__global__ __launch_bounds__(256) void fd_f0_kernel(int n_users, int n_items, const unsigned long long *__restrict__ pri, long long *__restrict__ info)
{
    __shared__ unsigned long long red[4];
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < n_items; i += 256) s += pri[(size_t)n_users + i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) info[3] = (long long)s;
}

RK_EXPORT int rk_fd_init(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                         const uint32_t *wtab, uint32_t *w_item, uint64_t *pri, int64_t *info, int32_t *status, void *stream)
{
    if (n_users < 0 || n_items < 0 || (int64_t)n_users + n_items < 1 || !rowptr || !col || !colptr || !wtab || !w_item || !pri || !info || !status)
        RK_FAIL(RK_EINVAL, "rk_fd_init: bad arguments");
    if ((int64_t)n_users + n_items > RK_FD_MAX_NODES)
        RK_FAIL(RK_EINVAL, "rk_fd_init: %lld nodes, at most %d", (long long)n_users + n_items, RK_FD_MAX_NODES);
    if (nnz < 0 || nnz >= RK_FD_MAX_NNZ) RK_FAIL(RK_EINVAL, "rk_fd_init: nnz = %lld outside 0..2^29 - 1", (long long)nnz);
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *bad = nullptr;
    RK_HIP(scratch.get(&bad, 2));
    RK_HIP(hipMemsetAsync(bad, 0xff, 2 * sizeof(unsigned long long), s));
    const int item_grid = (n_items + 255) / 256;
    if (n_items > 0) {
        hipLaunchKernelGGL(fd_check_kernel, dim3(item_grid), dim3(256), 0, s, n_users, n_items, colptr, wtab, bad);
        RK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fd_status_kernel, dim3(1), dim3(1), 0, s, bad, status);
    RK_CHECK_LAUNCH();
    int32_t h[2] = {0, 0};
    RK_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    if (h[0] == RK_FD_BAD_DEGREE) RK_FAIL(RK_EINVAL, "rk_fd_init: rule %d (a column length outside 0..n_users), first at item %d", h[0], h[1]);
    if (h[0]) RK_FAIL(RK_EINVAL, "rk_fd_init: rule %d (a weight outside 1..2^24), first at wtab[%d]", h[0], h[1]);
    if (n_items > 0) {
        hipLaunchKernelGGL(fd_item_kernel, dim3(item_grid), dim3(256), 0, s, n_users, n_items, colptr, wtab, w_item,
                           reinterpret_cast<unsigned long long *>(pri));
        RK_CHECK_LAUNCH();
    }
    if (n_users > 0) {
        hipLaunchKernelGGL(fd_user_kernel, dim3((n_users + 3) / 4), dim3(256), 0, s, n_users, n_items, (long long)nnz, rowptr, col, w_item,
                           reinterpret_cast<unsigned long long *>(pri));
        RK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fd_f0_kernel, dim3(1), dim3(256), 0, s, n_users, n_items, reinterpret_cast<const unsigned long long *>(pri),
                       reinterpret_cast<long long *>(info));
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---------------------------------------------------------------------------------------------------------------- rk_fd_peel
// the least (pri, id) of the wave's 64 pairs, in every lane
__device__ __forceinline__ void fd_wave_min(unsigned long long &p, int &id)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long q = __shfl_xor(p, o, 64);
        const int j = __shfl_xor(id, o, 64);
        if (q < p || (q == p && j < id)) {
            p = q;
            id = j;
        }
    }
}

// fa * nb > fb * na, exactly
__device__ __forceinline__ bool fd_denser(unsigned long long fa, unsigned long long na, unsigned long long fb, unsigned long long nb)
{
    const unsigned long long ah = __umul64hi(fa, nb), al = fa * nb, bh = __umul64hi(fb, na), bl = fb * na;
    return ah > bh || (ah == bh && al > bl);
}

struct FdLds {
    unsigned long long *pri;   // [total]
    unsigned long long *red;   // [kFdWaves]
    int *id;                   // [total]
    int *list;                 // [total]: the flagged blocks of level l from off[l] on
    unsigned *bits;            // [ceil(total / 32)]: entry off[l] + b is on its level's list
    int *cnt;                  // [2][kFdMaxLevels]: the lists' lengths, by the step's parity
};

// put entry b of level l on its list, once
__device__ __forceinline__ void fd_flag(const FdLds &m, const FdShape &sh, int par, int l, int b)
{
    const int e = sh.off[l] + b;
    const unsigned bit = 1u << (e & 31);
    if (!(atomicOr(&m.bits[e >> 5], bit) & bit)) m.list[sh.off[l] + atomicAdd(&m.cnt[par * kFdMaxLevels + l], 1)] = b;
}

// entry b of level l from its 64 children (leaves in global memory for level 0), by one wave; the result in every lane
__device__ __forceinline__ void fd_reduce(const FdLds &m, const FdShape &sh, int n_nodes, const unsigned long long *pri, int l, int b, int lane,
                                          unsigned long long *p_out, int *id_out)
{
    const int c = b * 64 + lane;
    unsigned long long p = kFdRemoved;
    int id = INT_MAX;
    if (l == 0) {
        if (c < n_nodes) {
            p = pri[c];
            id = c;
        }
    } else if (c < sh.nb[l - 1]) {
        p = m.pri[sh.off[l - 1] + c];
        id = m.id[sh.off[l - 1] + c];
    }
    *p_out = p;                                                     // the lane's own child, before the reduction
    fd_wave_min(p, id);
    if (lane == 0) {
        m.pri[sh.off[l] + b] = p;
        m.id[sh.off[l] + b] = id;
    }
    *id_out = id;
}

__global__ __launch_bounds__(kFdThreads) void fd_peel_kernel(int n_users, int n_items, long long nnz, const int *__restrict__ rowptr,
                                                             const int *__restrict__ col, const int *__restrict__ colptr,
                                                             const int *__restrict__ crow, const unsigned *__restrict__ w_item,
                                                             unsigned long long *pri, int *__restrict__ order, int *__restrict__ step_of,
                                                             unsigned long long *__restrict__ f_trace, long long *__restrict__ info, int t0, int t1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fd_lds[];
    const int n_nodes = n_users + n_items;
    const FdShape sh = fd_shape(n_nodes);
    FdLds m;
    m.pri = reinterpret_cast<unsigned long long *>(fd_lds);
    m.red = m.pri + sh.total;                                       // the 8-byte words first
    m.id = reinterpret_cast<int *>(m.red + kFdWaves);
    m.list = m.id + sh.total;
    m.bits = reinterpret_cast<unsigned *>(m.list + sh.total);
    m.cnt = reinterpret_cast<int *>(m.bits + (sh.total + 31) / 32);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- the hierarchy from pri as it stands, and f = the alive users' priorities
    for (int j = tid; j < (sh.total + 31) / 32; j += kFdThreads) m.bits[j] = 0u;
    if (tid < 2 * kFdMaxLevels) m.cnt[tid] = 0;
    unsigned long long fsum = 0;
    for (int b = wave; b < sh.nb[0]; b += kFdWaves) {
        unsigned long long own;
        int id;
        fd_reduce(m, sh, n_nodes, pri, 0, b, lane, &own, &id);
        if (b * 64 + lane < n_users && own != kFdRemoved) fsum += own;
    }
    fsum = wave_sum(fsum);
    if (lane == 0) m.red[wave] = fsum;
    __syncthreads();
#pragma unroll
    for (int l = 1; l < kFdMaxLevels; ++l) {
        if (l >= sh.levels) break;
        for (int b = wave; b < sh.nb[l]; b += kFdWaves) {
            unsigned long long own;
            int id;
            fd_reduce(m, sh, n_nodes, pri, l, b, lane, &own, &id);
        }
        __syncthreads();
    }
    unsigned long long f = 0;
#pragma unroll
    for (int q = 0; q < kFdWaves; ++q) f += m.red[q];
    unsigned long long best_f = 0, best_n = 1;
    int best_t = 0;
    if (t0 > 0) {
        best_t = (int)info[0];
        best_f = (unsigned long long)info[1];
        best_n = (unsigned long long)info[2];
    } else if (tid == 0) {
        info[3] = (long long)f;
    }
    const int root = sh.total - 1;                                  // the last level is one entry

#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        const int par = t & 1;
        const unsigned long long pv = m.pri[root];
        const int v = m.id[root];
        const unsigned long long n_t = (unsigned long long)(n_nodes - t);
        if (t == 0 || fd_denser(f, n_t, best_f, best_n)) {          // strict: the earliest maximum stays
            best_t = t;
            best_f = f;
            best_n = n_t;
        }
        const bool valid = (unsigned)v < (unsigned)n_nodes;         // always, while pri is what rk_fd_init wrote
        if (tid == 0) {
            order[t] = v;
            if (f_trace) f_trace[t] = f;
            if (valid) {
                step_of[v] = t;
                pri[v] = kFdRemoved;
                fd_flag(m, sh, par, 0, v >> 6);
            }
            for (int l = 0; l < kFdMaxLevels; ++l) m.cnt[(par ^ 1) * kFdMaxLevels + l] = 0;   // read last before the previous step's last barrier
        }
        if (pv != kFdRemoved) f -= pv;
        if (valid && v < n_users) {
            const long long beg = max((long long)rowptr[v], 0LL), end = min((long long)rowptr[v + 1], nnz);
            for (long long e = beg + tid; e < end; e += kFdThreads) {
                const int i = col[e];
                if ((unsigned)i >= (unsigned)n_items) continue;
                const int node = n_users + i;
                const unsigned long long p = pri[node];
                if (p == kFdRemoved) continue;
                pri[node] = p - w_item[i];
                fd_flag(m, sh, par, 0, node >> 6);
            }
        } else if (valid) {
            const int i = v - n_users;
            const unsigned long long w = w_item[i];
            const long long beg = max((long long)colptr[i], 0LL), end = min((long long)colptr[i + 1], nnz);
            for (long long e = beg + tid; e < end; e += kFdThreads) {
                const int u = crow[e];
                if ((unsigned)u >= (unsigned)n_users) continue;
                const unsigned long long p = pri[u];
                if (p == kFdRemoved) continue;
                pri[u] = p - w;
                fd_flag(m, sh, par, 0, u >> 6);
            }
        }
        __syncthreads();                                            // pri and the flags of this step are the workgroup's to read
        {                                                           // level 0: the leaves of kFdBatch blocks are loaded before the first is reduced
            const int n_flagged = m.cnt[par * kFdMaxLevels];
            for (int j = wave; j < n_flagged; j += kFdWaves * kFdBatch) {
                unsigned long long p[kFdBatch];
                int b[kFdBatch];
#pragma unroll
                for (int k = 0; k < kFdBatch; ++k) {
                    const int jj = j + k * kFdWaves;
                    b[k] = jj < n_flagged ? m.list[jj] : -1;        // the same in every lane of the wave
                    const int c = b[k] * 64 + lane;
                    p[k] = (b[k] >= 0 && c < n_nodes) ? pri[c] : kFdRemoved;
                }
#pragma unroll
                for (int k = 0; k < kFdBatch; ++k) {
                    if (b[k] < 0) continue;
                    const int c = b[k] * 64 + lane;
                    int id = c < n_nodes ? c : INT_MAX;
                    fd_wave_min(p[k], id);
                    if (lane == 0) {
                        m.pri[b[k]] = p[k];
                        m.id[b[k]] = id;
                        atomicAnd(&m.bits[b[k] >> 5], ~(1u << (b[k] & 31)));
                        if (sh.levels > 1) fd_flag(m, sh, par, 1, b[k] >> 6);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int l = 1; l < kFdMaxLevels; ++l) {
            if (l >= sh.levels) break;                              // the same in every thread
            const int n_flagged = m.cnt[par * kFdMaxLevels + l];
            for (int j = wave; j < n_flagged; j += kFdWaves) {
                const int b = m.list[sh.off[l] + j];
                unsigned long long own;
                int id;
                fd_reduce(m, sh, n_nodes, pri, l, b, lane, &own, &id);
                if (lane == 0) {
                    const int e = sh.off[l] + b;
                    atomicAnd(&m.bits[e >> 5], ~(1u << (e & 31)));
                    if (l + 1 < sh.levels) fd_flag(m, sh, par, l + 1, b >> 6);
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        info[0] = best_t;
        info[1] = (long long)best_f;
        info[2] = (long long)best_n;
    }
}

RK_EXPORT int rk_fd_peel_ex(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                            const int32_t *crow, const uint32_t *w_item, uint64_t *pri, int32_t *order, int32_t *step_of, uint64_t *f_trace,
                            int64_t *info, int32_t steps_per_launch, void *stream)
{
    if (n_users < 0 || n_items < 0 || (int64_t)n_users + n_items < 1 || !rowptr || !col || !colptr || !crow || !w_item || !pri || !order ||
        !step_of || !info)
        RK_FAIL(RK_EINVAL, "rk_fd_peel: bad arguments");
    if ((int64_t)n_users + n_items > RK_FD_MAX_NODES)
        RK_FAIL(RK_EINVAL, "rk_fd_peel: %lld nodes, at most %d (the hierarchy of minima lives in one workgroup's LDS)",
                (long long)n_users + n_items, RK_FD_MAX_NODES);
    if (nnz < 0 || nnz >= RK_FD_MAX_NNZ) RK_FAIL(RK_EINVAL, "rk_fd_peel: nnz = %lld outside 0..2^29 - 1", (long long)nnz);
    if (steps_per_launch < 1) RK_FAIL(RK_EINVAL, "rk_fd_peel: steps_per_launch = %d, at least 1", steps_per_launch);
    hipStream_t s = (hipStream_t)stream;
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fd_peel_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxBytes - 64));
        attr_once.done(attr_dev);
    }
    const int n_nodes = n_users + n_items;
    const size_t lds = fd_lds_bytes(fd_shape(n_nodes).total);
    for (int t0 = 0; t0 < n_nodes;) {
        const int t1 = (int)(n_nodes - t0 > steps_per_launch ? t0 + steps_per_launch : n_nodes);
        hipLaunchKernelGGL(fd_peel_kernel, dim3(1), dim3(kFdThreads), lds, s, n_users, n_items, (long long)nnz, rowptr, col, colptr, crow, w_item,
                           reinterpret_cast<unsigned long long *>(pri), order, step_of, reinterpret_cast<unsigned long long *>(f_trace),
                           reinterpret_cast<long long *>(info), t0, t1);
        RK_CHECK_LAUNCH();
        t0 = t1;
    }
    return RK_OK;
}

RK_EXPORT int rk_fd_peel(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                         const int32_t *crow, const uint32_t *w_item, uint64_t *pri, int32_t *order, int32_t *step_of, uint64_t *f_trace,
                         int64_t *info, void *stream)
{
    return rk_fd_peel_ex(n_users, n_items, nnz, rowptr, col, colptr, crow, w_item, pri, order, step_of, f_trace, info, RK_FD_STEPS_PER_LAUNCH,
                         stream);
}
