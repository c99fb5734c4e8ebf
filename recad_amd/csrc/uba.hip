// UBA's target-user budget selection (recad/model/attacker/uba.py:81-140) on the device.  The reference redraws the target
// users' ratings, appends add_num copies of each redrawn row to a dense train matrix, builds the dense (M+N)^2 bipartite
// matrix of the result, "cubes" it and asks whether selected_ids[0] is among each target user's ten best items -- ten times
// for each add_num = 1..budget.  Here
//   * the redrawn rows live in a side CSR of n_targets short rows (rk_uba_redraw, uba.py:86-91); the rating data itself is
//     never written (the reference overwrites the first target user's row in place: a documented deviation);
//   * the appended copies are never made: a target user's row simply weighs 1 + add_num (rk_uba_scores);
//   * the score rows are the redrawn rows cubed (RK_UBA_ELEMENTWISE: uba.py:99 as written, `*` is elementwise) or rows
//     target_user_ids of (E @ E @ E)[:M, M:] (RK_UBA_MATRIX: what uba.py:95-100 set out to compute).  With r'_v the rows of
//     the redrawn matrix and c_v = 1 + add_num for a target user, 1 otherwise, the latter is
//         x_t = sum_v c_v <r'_v, r'_t> r'_v
//     in three kernels: the weights w_t[v] = c_v <r'_v, r'_t> by walking the CSC columns of the items t rated (integer LDS
//     atomics, or global ones when n_users is above RK_UBA_LDS_USERS), then one wave per (t, item) gathers
//     sum_v w_t[v] r'_v[item] over the item's CSC column, then the counts against x_t[s].  Every term is an integer and the
//     sums are int64, so the result is exact and the same on every run whatever the order of the atomics;
//   * the top-ten test (uba.py:102-113) is a count: s is in when n_greater + n_equal_before < 10 (rk_uba_scores);
//   * the budget x 10 loop runs on the stream and prob_mat is read back once (rk_uba_prob, uba.py:119-140).
// A target user's stale row in the CSC is cancelled, not skipped: its weight in w_t is set to 0 and the redrawn rows are added
// from the side CSR, one lane per target user (RK_UBA_MAX_TARGETS is the wave size).
#include <algorithm>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
typedef unsigned long long u64;

struct UbaTargets {
    int n, pad;
    int users[RK_UBA_MAX_TARGETS];
};

// [b, e) of side row t, clamped into [0, side_cap)
__device__ __forceinline__ void side_row(const int *__restrict__ side_ptr, int t, int side_cap, int *b, int *e)
{
    const int lo = side_ptr[t], hi = side_ptr[t + 1];
    *b = min(max(lo, 0), side_cap);
    *e = min(max(hi, *b), side_cap);
}

// ---------------------------------------------------------------- the redraw (uba.py:86-91)
// One workgroup per target user.  Every workgroup computes all n_targets row lengths (rated items, plus one when s is not among
// them) so that each knows its own offset and all of them agree on whether the rows fit: when a row pointer is out of order
// or the rows need more than side_cap entries, *status becomes 1 and nothing else is written.
__global__ __launch_bounds__(kBlock) void redraw_kernel(UbaTargets T, long long nnz, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        int s, u64 stream_id, const int *__restrict__ draws, u64 seed, int side_cap,
                                                        int *__restrict__ side_ptr, int *__restrict__ side_col, int *__restrict__ side_val,
                                                        int *__restrict__ status)
{
    __shared__ int len[RK_UBA_MAX_TARGETS], row_b[RK_UBA_MAX_TARGETS], spos[RK_UBA_MAX_TARGETS], off[RK_UBA_MAX_TARGETS + 1];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (tid < T.n) {
        const int u = T.users[tid];
        const long long b = rowptr[u], e = rowptr[u + 1];
        if (b < 0 || e < b || e > nnz) {
            len[tid] = -1;
            row_b[tid] = spos[tid] = 0;
        } else {
            const int p = rk_lower_bound(col, (int)b, (int)e, s);
            const bool has = p < (int)e && col[p] == s;
            len[tid] = (int)(e - b) + (has ? 0 : 1);
            row_b[tid] = (int)b;
            spos[tid] = has ? -(p - (int)b) - 1 : p - (int)b;      // s sits at this position of the redrawn row; negative: it was rated
        }
    }
    __syncthreads();
    if (tid == 0) {
        long long total = 0;
        bool ok = true;
        for (int i = 0; i < T.n; ++i) {
            off[i] = (int)total;
            ok = ok && len[i] > 0;
            total += ok ? len[i] : 0;
            ok = ok && total <= side_cap;
        }
        off[T.n] = ok ? (int)total : -1;
    }
    __syncthreads();
    if (off[T.n] < 0) {
        if (tid == 0 && t == 0) *status = 1;
        return;
    }
    const int o = off[t], n = len[t], b0 = row_b[t];
    const bool has = spos[t] < 0;
    const int ps = has ? -spos[t] - 1 : spos[t];
    for (int k = tid; k < n; k += kBlock) {
        int c = s, v = 5;                                          // uba.py:91
        if (k != ps) {
            c = col[b0 + (has || k < ps ? k : k - 1)];
            v = draws ? draws[o + k]                               // uba.py:90: random.randint(1, 5)
                      : 1 + (int)(((rk_draw_key(seed, stream_id, t, k) >> 32) * 5ULL) >> 32);
        }
        side_col[o + k] = c;
        side_val[o + k] = v;
    }
    if (tid == 0) side_ptr[t] = o;
    if (tid == 0 && t == T.n - 1) side_ptr[T.n] = o + n;
}

// ---------------------------------------------------------------- the score rows, elementwise (uba.py:99 as written)
__global__ __launch_bounds__(kBlock) void cube_kernel(int n_items, int side_cap, const int *__restrict__ side_ptr, const int *__restrict__ side_col,
                                                      const int *__restrict__ side_val, double *__restrict__ x)
{
    const int t = blockIdx.x;
    int sb, se;
    side_row(side_ptr, t, side_cap, &sb, &se);
    for (int j = blockIdx.y * kBlock + threadIdx.x; j < n_items; j += gridDim.y * kBlock) {
        const int k = rk_find_sorted(side_col, sb, se, j);
        const double v = k >= 0 ? (double)side_val[k] : 0.0;
        x[(long long)t * n_items + j] = v * v * v;
    }
}

// ---------------------------------------------------------------- the score rows, three hops (uba.py:95-100 as meant)
// w_t[v] = <r_v, r'_t> over the CSC columns of the items in r'_t, for every user v; then the target users' entries become 0
// and wt[t, t2] = (1 + b) <r'_t2, r'_t> takes their place.  kLds: w_t is accumulated in LDS and copied out at the end.
template <bool kLds>
__global__ __launch_bounds__(kBlock) void weights_kernel(UbaTargets T, int n_users, int n_items, long long nnz, const int *__restrict__ colptr,
                                                         const int *__restrict__ crow, const float *__restrict__ cval, int side_cap,
                                                         const int *__restrict__ side_ptr, const int *__restrict__ side_col,
                                                         const int *__restrict__ side_val, int c_target, u64 *__restrict__ gw,
                                                         long long *__restrict__ wt)
{
    extern __shared__ u64 lds_w[];
    const int t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    u64 *out = gw + (long long)t * n_users;
    u64 *w = kLds ? lds_w : out;
    for (int v = tid; v < n_users; v += kBlock) w[v] = 0ULL;
    __threadfence_block();
    __syncthreads();
    int sb, se;
    side_row(side_ptr, t, side_cap, &sb, &se);
    for (int k = sb + wave; k < se; k += kWaves) {
        const int j = side_col[k], a = side_val[k];
        if ((unsigned)j >= (unsigned)n_items) continue;
        const long long cb = min(max((long long)colptr[j], 0LL), nnz), ce = min(max((long long)colptr[j + 1], cb), nnz);
        for (long long p = cb + lane; p < ce; p += 64) {
            const int v = crow[p];
            if ((unsigned)v < (unsigned)n_users) atomicAdd(&w[v], (u64)((long long)a * (long long)(int)cval[p]));
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int t2 = tid; t2 < T.n; t2 += kBlock) {
        int b2, e2, i = sb;
        side_row(side_ptr, t2, side_cap, &b2, &e2);
        long long dot = 0;
        while (i < se && b2 < e2) {                                // both rows ascend by item id
            const int ci = side_col[i], c2 = side_col[b2];
            if (ci == c2) dot += (long long)side_val[i] * (long long)side_val[b2];
            i += ci <= c2 ? 1 : 0;
            b2 += c2 <= ci ? 1 : 0;
        }
        wt[t * T.n + t2] = (long long)c_target * dot;
        w[T.users[t2]] = 0ULL;
    }
    if (kLds) {
        __syncthreads();
        for (int v = tid; v < n_users; v += kBlock) out[v] = w[v];
    }
}

// x[t, j] = sum_v w_t[v] r_v[j] over CSC column j, plus the target users' redrawn rows: one wave per (t, j), lane l looks j up in
// side row l.  kLds: w_t is staged in LDS first.
template <bool kLds>
__global__ __launch_bounds__(kBlock) void gather_kernel(int n_targets, int n_users, int n_items, long long nnz, const int *__restrict__ colptr,
                                                        const int *__restrict__ crow, const float *__restrict__ cval, int side_cap,
                                                        const int *__restrict__ side_ptr, const int *__restrict__ side_col,
                                                        const int *__restrict__ side_val, const u64 *__restrict__ gw,
                                                        const long long *__restrict__ wt, double *__restrict__ x)
{
    extern __shared__ u64 lds_w[];
    const int t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u64 *w = gw + (long long)t * n_users;
    if (kLds) {
        for (int v = tid; v < n_users; v += kBlock) lds_w[v] = w[v];
        __syncthreads();
        w = lds_w;
    }
    int tb = 0, te = 0;
    long long wl = 0;
    if (lane < n_targets) {
        side_row(side_ptr, lane, side_cap, &tb, &te);
        wl = wt[t * n_targets + lane];
    }
    for (int j = blockIdx.y * kWaves + wave; j < n_items; j += gridDim.y * kWaves) {
        const long long cb = min(max((long long)colptr[j], 0LL), nnz), ce = min(max((long long)colptr[j + 1], cb), nnz);
        long long acc = 0;
        for (long long p = cb + lane; p < ce; p += 64) {
            const int v = crow[p];
            if ((unsigned)v < (unsigned)n_users) acc += (long long)w[v] * (long long)(int)cval[p];
        }
        const int k = rk_find_sorted(side_col, tb, te, j);
        if (k >= 0) acc += wl * (long long)side_val[k];
        acc = wave_sum(acc);
        if (lane == 0) x[(long long)t * n_items + j] = (double)acc;
    }
}

// ---------------------------------------------------------------- the top-ten test as counts (uba.py:102-113)
// counts[0, t] = #{j : x[j] > x[s]}, counts[1, t] = #{j != s : x[j] == x[s]}, counts[2, t] = those of them with j < s.  With hits:
// hits[t, column] += n_greater + n_equal_before < RK_UBA_TOPN, *ties += n_greater < RK_UBA_TOPN <= n_greater + n_equal.
__global__ __launch_bounds__(kBlock) void count_kernel(int n_targets, int n_items, int s, const double *__restrict__ x, int *__restrict__ counts,
                                                       int *__restrict__ hits, int ld_hits, int column, int *__restrict__ ties)
{
    __shared__ int red[kWaves];
    const int t = blockIdx.x;
    const double *row = x + (long long)t * n_items;
    const double xs = row[s];
    int g = 0, e = 0, eb = 0;
    for (int j = threadIdx.x; j < n_items; j += kBlock) {
        const double v = row[j];
        g += v > xs ? 1 : 0;
        e += (v == xs && j != s) ? 1 : 0;
        eb += (v == xs && j < s) ? 1 : 0;
    }
    g = block_sum_256(g, red);
    e = block_sum_256(e, red);
    eb = block_sum_256(eb, red);
    if (threadIdx.x == 0) {
        if (counts) {
            counts[t] = g;
            counts[n_targets + t] = e;
            counts[2 * n_targets + t] = eb;
        }
        if (hits) {
            hits[t * ld_hits + column] += g + eb < RK_UBA_TOPN ? 1 : 0;      // one writer per (t, column), launches in stream order
            if (g < RK_UBA_TOPN && g + e >= RK_UBA_TOPN) atomicAdd(ties, 1);
        }
    }
}

// ---------------------------------------------------------------- host side
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// one scratch buffer of a call, carved up: the only place that knows the sizes
struct UbaLayout {
    size_t side_ptr, side_col, side_val, counts, hits, w, wt, x, bytes;
    UbaLayout(int n_users, int n_items, int n_targets, int side_cap, int budget)
    {
        size_t o = 0;
        auto take = [&o](size_t n) { const size_t at = o; o += align256(n); return at; };
        side_ptr = take(sizeof(int) * ((size_t)n_targets + 1));
        side_col = take(sizeof(int) * (size_t)side_cap);
        side_val = take(sizeof(int) * (size_t)side_cap);
        counts = take(sizeof(int) * 3 * (size_t)n_targets);
        hits = take(sizeof(int) * ((size_t)n_targets * budget + 2));        // then the tie count and the redraw's status
        w = take(sizeof(u64) * (size_t)n_targets * n_users);
        wt = take(sizeof(long long) * (size_t)n_targets * n_targets);
        x = take(sizeof(double) * (size_t)n_targets * n_items);
        bytes = o;
    }
};

// the refusals every entry shares; fills T.  what: the entry's name
int check_targets(const char *what, int n_users, int n_items, const int32_t *target_users, int n_targets, int s, int b, int side_cap, UbaTargets *T)
{
    if (n_users <= 0 || n_items <= 0 || !target_users) RK_FAIL(RK_EINVAL, "%s: bad arguments (n_users %d, n_items %d)", what, n_users, n_items);
    if (n_targets <= 0 || n_targets > RK_UBA_MAX_TARGETS)
        RK_FAIL(RK_EINVAL, "%s: %d target users (1..%d)", what, n_targets, RK_UBA_MAX_TARGETS);
    if (s < 0 || s >= n_items) RK_FAIL(RK_EINVAL, "%s: selected id %d outside [0, %d)", what, s, n_items);
    if (b < 1 || b > RK_UBA_MAX_BUDGET) RK_FAIL(RK_EINVAL, "%s: budget step %d (1..%d)", what, b, RK_UBA_MAX_BUDGET);
    if (side_cap < n_targets || (long long)side_cap > (long long)n_targets * n_items)
        RK_FAIL(RK_EINVAL, "%s: side_cap %d (%d..%lld)", what, side_cap, n_targets, (long long)n_targets * n_items);
    T->n = n_targets;
    T->pad = 0;
    for (int i = 0; i < RK_UBA_MAX_TARGETS; ++i) T->users[i] = 0;
    for (int i = 0; i < n_targets; ++i) {
        const int u = target_users[i];
        if (u < 0 || u >= n_users) RK_FAIL(RK_EINVAL, "%s: target user %d outside [0, %d)", what, u, n_users);
        for (int k = 0; k < i; ++k)
            if (T->users[k] == u) RK_FAIL(RK_EINVAL, "%s: target user %d is listed twice", what, u);
        T->users[i] = u;
    }
    return RK_OK;
}

// mode / path refusals; *lds = the weights live in LDS
int check_mode(const char *what, int n_users, int n_items, int n_targets, int b, int mode, int path, bool *lds)
{
    if (mode != RK_UBA_ELEMENTWISE && mode != RK_UBA_MATRIX) RK_FAIL(RK_EINVAL, "%s: mode %d", what, mode);
    if (path != RK_UBA_PATH_AUTO && path != RK_UBA_PATH_LDS && path != RK_UBA_PATH_WORK) RK_FAIL(RK_EINVAL, "%s: path %d", what, path);
    if (path == RK_UBA_PATH_LDS && n_users > RK_UBA_LDS_USERS)
        RK_FAIL(RK_EINVAL, "%s: the LDS path holds at most %d users (n_users %d)", what, RK_UBA_LDS_USERS, n_users);
    // a score is at most (users + appended rows) * 25 n_items * 5: every int64 sum must also be an exact double
    if (mode == RK_UBA_MATRIX && ((double)n_users + (double)n_targets * b) * 125.0 * (double)n_items > 0x1.0p53)
        RK_FAIL(RK_EINVAL, "%s: %d users x %d items can exceed 2^53 in a three-hop score", what, n_users, n_items);
    *lds = path == RK_UBA_PATH_LDS || (path == RK_UBA_PATH_AUTO && n_users <= RK_UBA_LDS_USERS);
    return RK_OK;
}

struct UbaCsc {
    long long nnz;
    const int *colptr, *crow;
    const float *cval;
};

// the score rows of one redraw into x, then the counts (and hits / ties when given)
int launch_scores(const UbaTargets &T, int n_users, int n_items, const UbaCsc &c, int side_cap, const int *side_ptr, const int *side_col,
                  const int *side_val, int s, int b, int mode, bool lds, u64 *w, long long *wt, double *x, int *counts, int *hits, int ld_hits,
                  int *ties, hipStream_t st)
{
    if (mode == RK_UBA_ELEMENTWISE) {
        hipLaunchKernelGGL(cube_kernel, dim3(T.n, std::min((n_items + kBlock - 1) / kBlock, 64)), dim3(kBlock), 0, st, n_items, side_cap, side_ptr,
                           side_col, side_val, x);
        RK_CHECK_LAUNCH();
    } else {
        const size_t smem = lds ? sizeof(u64) * (size_t)n_users : 0;
        const dim3 ggrid(T.n, std::max(1, std::min((n_items + kWaves - 1) / kWaves, 2048 / T.n)));
        if (lds) {
            hipLaunchKernelGGL(weights_kernel<true>, dim3(T.n), dim3(kBlock), smem, st, T, n_users, n_items, c.nnz, c.colptr, c.crow, c.cval, side_cap,
                               side_ptr, side_col, side_val, 1 + b, w, wt);
            RK_CHECK_LAUNCH();
            hipLaunchKernelGGL(gather_kernel<true>, ggrid, dim3(kBlock), smem, st, T.n, n_users, n_items, c.nnz, c.colptr, c.crow, c.cval, side_cap,
                               side_ptr, side_col, side_val, (const u64 *)w, (const long long *)wt, x);
        } else {
            hipLaunchKernelGGL(weights_kernel<false>, dim3(T.n), dim3(kBlock), 0, st, T, n_users, n_items, c.nnz, c.colptr, c.crow, c.cval, side_cap,
                               side_ptr, side_col, side_val, 1 + b, w, wt);
            RK_CHECK_LAUNCH();
            hipLaunchKernelGGL(gather_kernel<false>, ggrid, dim3(kBlock), 0, st, T.n, n_users, n_items, c.nnz, c.colptr, c.crow, c.cval, side_cap,
                               side_ptr, side_col, side_val, (const u64 *)w, (const long long *)wt, x);
        }
        RK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(count_kernel, dim3(T.n), dim3(kBlock), 0, st, T.n, n_items, s, (const double *)x, counts, hits, ld_hits, b - 1, ties);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

}  // namespace

static_assert(RK_UBA_MAX_TARGETS == 64, "gather_kernel gives one lane of a wave to each target user");
static_assert(sizeof(u64) * RK_UBA_LDS_USERS <= 64 * 1024, "the LDS weights must fit the default dynamic LDS limit");

RK_EXPORT int rk_uba_workspace_bytes(int32_t n_users, int32_t n_items, int32_t n_targets, int32_t side_cap, int32_t budget, int64_t *bytes)
{
    if (n_users <= 0 || n_items <= 0 || n_targets <= 0 || n_targets > RK_UBA_MAX_TARGETS || side_cap < n_targets ||
        (long long)side_cap > (long long)n_targets * n_items || budget < 1 || budget > RK_UBA_MAX_BUDGET || !bytes)
        RK_FAIL(RK_EINVAL, "rk_uba_workspace_bytes: bad arguments (n_users %d, n_items %d, %d target users, side_cap %d, budget %d)", n_users,
                n_items, n_targets, side_cap, budget);
    *bytes = (int64_t)UbaLayout(n_users, n_items, n_targets, side_cap, budget).bytes;
    return RK_OK;
}

RK_EXPORT int rk_uba_redraw(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *target_users,
                            int32_t n_targets, int32_t s, int32_t b, int32_t trial, const int32_t *draws, uint64_t seed, int32_t side_cap,
                            int32_t *side_ptr, int32_t *side_col, int32_t *side_val, int32_t *status, void *stream)
{
    UbaTargets T;
    const int rc = check_targets("rk_uba_redraw", n_users, n_items, target_users, n_targets, s, b, side_cap, &T);
    if (rc != RK_OK) return rc;
    if (nnz < 0 || trial < 0 || !rowptr || (nnz > 0 && !col) || !side_ptr || !side_col || !side_val || !status)
        RK_FAIL(RK_EINVAL, "rk_uba_redraw: bad arguments (nnz %lld, trial %d)", (long long)nnz, trial);
    hipLaunchKernelGGL(redraw_kernel, dim3(n_targets), dim3(kBlock), 0, (hipStream_t)stream, T, (long long)nnz, rowptr, col, s,
                       ((u64)(uint32_t)b << 32) | (u64)(uint32_t)trial, draws, (u64)seed, side_cap, side_ptr, side_col, side_val, status);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_uba_scores(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *colptr, const int32_t *crow, const float *cval,
                            const int32_t *target_users, int32_t n_targets, const int32_t *side_ptr, const int32_t *side_col,
                            const int32_t *side_val, int32_t side_cap, int32_t s, int32_t b, int32_t mode, int32_t path, int32_t *counts, double *x,
                            void *stream)
{
    UbaTargets T;
    bool lds = false;
    int rc = check_targets("rk_uba_scores", n_users, n_items, target_users, n_targets, s, b, side_cap, &T);
    if (rc == RK_OK) rc = check_mode("rk_uba_scores", n_users, n_items, n_targets, b, mode, path, &lds);
    if (rc != RK_OK) return rc;
    if (nnz < 0 || !colptr || (nnz > 0 && (!crow || !cval)) || !side_ptr || !side_col || !side_val || !counts)
        RK_FAIL(RK_EINVAL, "rk_uba_scores: bad arguments (nnz %lld)", (long long)nnz);
    hipStream_t st = (hipStream_t)stream;
    const UbaLayout L(n_users, n_items, n_targets, side_cap, 1);
    RkScratch scratch(st);
    char *work = nullptr;
    RK_HIP(scratch.get(&work, L.bytes));
    const UbaCsc c{(long long)nnz, colptr, crow, cval};
    return launch_scores(T, n_users, n_items, c, side_cap, side_ptr, side_col, side_val, s, b, mode, lds, (u64 *)(work + L.w),
                         (long long *)(work + L.wt), x ? x : (double *)(work + L.x), counts, nullptr, 0, nullptr, st);
}

RK_EXPORT int rk_uba_prob(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                          const int32_t *crow, const float *cval, const int32_t *target_users, int32_t n_targets, int32_t s, int32_t budget,
                          int32_t mode, int32_t path, const int32_t *draws, uint64_t seed, int32_t side_cap, double *prob_mat, int32_t *n_tie,
                          void *stream)
{
    UbaTargets T;
    bool lds = false;
    int rc = check_targets("rk_uba_prob", n_users, n_items, target_users, n_targets, s, budget, side_cap, &T);
    if (rc == RK_OK) rc = check_mode("rk_uba_prob", n_users, n_items, n_targets, budget, mode, path, &lds);
    if (rc != RK_OK) return rc;
    if (nnz < 0 || !rowptr || !colptr || (nnz > 0 && (!col || !crow || !cval)) || !prob_mat || !n_tie)
        RK_FAIL(RK_EINVAL, "rk_uba_prob: bad arguments (nnz %lld)", (long long)nnz);
    hipStream_t st = (hipStream_t)stream;
    const UbaLayout L(n_users, n_items, n_targets, side_cap, budget);
    RkScratch scratch(st);
    char *work = nullptr;
    RK_HIP(scratch.get(&work, L.bytes));
    int *side_ptr = (int *)(work + L.side_ptr), *side_col = (int *)(work + L.side_col), *side_val = (int *)(work + L.side_val);
    int *hits = (int *)(work + L.hits), *ties = hits + n_targets * budget, *status = ties + 1;
    RK_HIP(rk_zero_async(hits, sizeof(int) * ((size_t)n_targets * budget + 2), st));
    RK_HIP(rk_zero_async(side_ptr, sizeof(int) * ((size_t)n_targets + 1), st));      // a refused redraw leaves empty rows behind
    const UbaCsc c{(long long)nnz, colptr, crow, cval};
    for (int b = 1; b <= budget; ++b) {                                               // uba.py:122-123, add_num = b
        for (int trial = 0; trial < RK_UBA_TRIALS; ++trial) {                         // uba.py:127
            const int32_t *d = draws ? draws + ((size_t)(b - 1) * RK_UBA_TRIALS + trial) * (size_t)side_cap : nullptr;
            hipLaunchKernelGGL(redraw_kernel, dim3(n_targets), dim3(kBlock), 0, st, T, (long long)nnz, rowptr, col, s,
                               ((u64)(uint32_t)b << 32) | (u64)(uint32_t)trial, d, (u64)seed, side_cap, side_ptr, side_col, side_val, status);
            RK_CHECK_LAUNCH();
            rc = launch_scores(T, n_users, n_items, c, side_cap, side_ptr, side_col, side_val, s, b, mode, lds, (u64 *)(work + L.w),
                               (long long *)(work + L.wt), (double *)(work + L.x), nullptr, hits, budget, ties, st);
            if (rc != RK_OK) return rc;
        }
    }
    int host[RK_UBA_MAX_TARGETS * RK_UBA_MAX_BUDGET + 2];
    RK_HIP(hipMemcpyAsync(host, hits, sizeof(int) * ((size_t)n_targets * budget + 2), hipMemcpyDeviceToHost, st));   // the one read-back
    RK_HIP(hipStreamSynchronize(st));
    if (host[n_targets * budget + 1]) RK_FAIL(RK_EINVAL, "rk_uba_prob: the target users' rows do not fit side_cap %d, or a row pointer is out of order", side_cap);
    for (int i = 0; i < n_targets * budget; ++i) prob_mat[i] = (double)host[i] / (double)RK_UBA_TRIALS;          // uba.py:138
    *n_tie = host[n_targets * budget];
    return RK_OK;
}
