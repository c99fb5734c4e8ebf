// Average, segment and bandwagon attackers (recad/model/attacker/heuristic.py:85-325) on the device.  The reference
// computes its per-item means with one boolean mask over all ratings per distinct item (heuristic.py:94-98), ranks the
// items with a pandas groupby (heuristic.py:252-259) and writes dense attack_num x n_items profiles on the host; here
//   * one pass over the rating CSR gives every item's count and mean and the global mean, a second one the global
//     population standard deviation (rk_heur_item_stats).  The per-item sums are float64 ATOMICS: their order of
//     addition is not fixed, so item_mean can differ between two runs in the last bits (within count * 2^-52 * max|rating|
//     of the exact value, like any float64 summation order).  The counts are integers and the two global sums are reduced
//     per block and then in block order, so those are the same on every run;
//   * the k most rated items come from a radix sort of the integer keys (count << 32 | item id), so equal counts fall
//     larger id first and no count is ever rounded (rk_heur_popular);
//   * one workgroup builds one profile row: wave 0 draws (or reads) the fillers while the other waves start the zero fill,
//     then the few nonzeros are scattered over the filled row (rk_heur_generate).
// Random draws come from rk_mix64 keyed on (seed, stream, row, draw) like the AUSH sampler's: the stream is a per-call id.
#include <algorithm>
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPartials = 1024;

// ---------------------------------------------------------------- statistics (heuristic.py:91-98)
// pass 0: cnt[c] += 1, sum[c] += rating for every stored rating, partial[block] = the block's rating sum
// pass 1: partial[block] = the block's sum of (rating - global mean)^2
__global__ __launch_bounds__(kBlock) void stats_pass_kernel(int pass, long long nnz, int n_items, const int *__restrict__ col,
                                                            const float *__restrict__ val, int *__restrict__ cnt, double *__restrict__ sum,
                                                            const double *__restrict__ global, double *__restrict__ partial)
{
    __shared__ double red[kBlock / 64];
    const long long stride = (long long)gridDim.x * kBlock;
    const double mean = pass ? global[0] : 0.0;
    double acc = 0.0;
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < nnz; k += stride) {
        const double v = (double)val[k];
        if (pass) {
            acc += (v - mean) * (v - mean);
        } else {
            const int c = col[k];
            if ((unsigned)c < (unsigned)n_items) {
                atomicAdd(&cnt[c], 1);
                atomicAdd(&sum[c], v);
            }
            acc += v;
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// one block: global[pass] = mean of the ratings (pass 0) or their population standard deviation (pass 1); 0 without ratings
__global__ __launch_bounds__(kBlock) void stats_global_kernel(int pass, int n_partial, long long nnz, const double *__restrict__ partial,
                                                              double *__restrict__ global)
{
    __shared__ double red[kBlock / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < n_partial; b += kBlock) acc += partial[b];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        const double m = nnz > 0 ? acc / (double)nnz : 0.0;
        global[pass] = pass ? sqrt(m) : m;
    }
}

// item_mean = sum / count in place (0 where nobody rated), n_rated = #{count > 0}
__global__ __launch_bounds__(kBlock) void stats_item_kernel(int n_items, const int *__restrict__ cnt, double *__restrict__ mean,
                                                            int *__restrict__ n_rated)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int c = i < n_items ? cnt[i] : 0;
    if (i < n_items) mean[i] = c > 0 ? mean[i] / (double)c : 0.0;
    const int n = __popcll(__ballot(c > 0));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_rated, n);
}

// ---------------------------------------------------------------- popularity (heuristic.py:252-259)
__global__ void popular_keys_kernel(int n_items, const int *__restrict__ cnt, unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const int c = cnt[i];
    keys[i] = c > 0 ? (((unsigned long long)(unsigned)c << 32) | (unsigned long long)(unsigned)i) : 0ULL;
}

__global__ void popular_take_kernel(int n_items, int k, const unsigned long long *__restrict__ sorted, int *__restrict__ ids,
                                    int *__restrict__ counts, int *__restrict__ n_found)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const unsigned long long key = i < n_items ? sorted[i] : 0ULL;
    const int c = (int)(key >> 32);
    ids[i] = c > 0 ? (int)(key & 0xffffffffULL) : -1;
    counts[i] = c;
    if (c > 0) atomicAdd(n_found, 1);
}

// ---------------------------------------------------------------- profiles (heuristic.py:115-151, 191-220, 274-311)
struct HeurSets {
    int n_targets, n_sel, n_excl, pad;
    int targets[RK_HEUR_MAX_TARGETS];                       // in the caller's order, repeats kept
    int selected[RK_HEUR_MAX_SELECT];
    int excl[RK_HEUR_MAX_TARGETS + RK_HEUR_MAX_SELECT];     // targets U selected, ascending, distinct
};

// a standard normal from two 53-bit uniforms (Box-Muller in float64)
__device__ __forceinline__ double std_normal(unsigned long long a, unsigned long long b)
{
    const double u1 = (double)((a >> 11) + 1ULL) * 0x1.0p-53;   // (0, 1]
    const double u2 = (double)(b >> 11) * 0x1.0p-53;            // [0, 1)
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// One workgroup per row.  Wave 0 gets the row's filler columns into LDS -- the given draws, or filler_num distinct
// pool positions by Floyd's subset algorithm (position k of the sorted pool is item k plus the excluded ids at or below it)
// -- while waves 1..3 already zero the row; every element of the row is then written once as zero, and the nonzeros go on
// top.  A nonzero's address was zeroed by ANOTHER thread of this workgroup, so the scatter must come after the fill in
// memory order: the workgroup-scope fence and the barrier between them make every fill store happen-before every scatter
// store, and two stores to one address ordered by happens-before reach memory in that order.
__global__ __launch_bounds__(kBlock) void generate_kernel(int n_items, int F, int rate, HeurSets a, int mode, double gmean, double gstd,
                                                          const double *__restrict__ item_mean, const int *__restrict__ item_count,
                                                          const int *__restrict__ draw_cols, const double *__restrict__ draw_vals,
                                                          unsigned long long seed, unsigned long long stream, float *__restrict__ out)
{
    __shared__ int fcol[RK_HEUR_MAX_FILLER];
    const int r = blockIdx.x, t = threadIdx.x;
    float *o = out + (long long)r * n_items;
    if (t < 64) {
        if (draw_cols) {
            for (int k = t; k < F; k += 64) fcol[k] = draw_cols[(long long)r * F + k];
        } else {
            // Floyd: for j = P - F .. P - 1 draw x uniform in [0, j]; take x, or j when x is already taken.  Every F-subset
            // of the P pool positions is equally likely.  Lane l keeps picks l, l + 64, ... in registers.
            constexpr int kPer = RK_HEUR_MAX_FILLER / 64;
            int mine[kPer];
#pragma unroll
            for (int m = 0; m < kPer; ++m) mine[m] = -1;
            const int P = n_items - a.n_excl;
            for (int k = 0; k < F; ++k) {
                const int j = P - F + k;
                const unsigned long long x = rk_draw_key(seed, stream, r, k);
                const int cand = (int)(((x >> 32) * (unsigned long long)(j + 1)) >> 32);
                bool hit = false;
#pragma unroll
                for (int m = 0; m < kPer; ++m) hit |= mine[m] == cand;
                const int pick = __any(hit) ? j : cand;
#pragma unroll
                for (int m = 0; m < kPer; ++m)
                    if (m == (k >> 6) && t == (k & 63)) mine[m] = pick;
            }
#pragma unroll
            for (int m = 0; m < kPer; ++m) {
                const int k = m * 64 + t;
                if (k < F) {
                    int c = mine[m];
                    for (int e = 0; e < a.n_excl; ++e) c += a.excl[e] <= c ? 1 : 0;
                    fcol[k] = c;
                }
            }
        }
    }
    // zero fill: scalar stores up to the first 16-byte boundary, 16-byte stores, scalar tail
    const int head = min(n_items, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(o) & 15u)) & 15u) >> 2));
    const int nvec = (n_items - head) >> 2;
    float4 *o4 = reinterpret_cast<float4 *>(o + head);
    if (t < head) o[t] = 0.f;
    for (int v = t; v < nvec; v += kBlock) o4[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = head + nvec * 4 + t; i < n_items; i += kBlock) o[i] = 0.f;
    __threadfence_block();
    __syncthreads();
    for (int k = t; k < F; k += kBlock) {
        const int c = fcol[k];
        double x = 1.0;                                          // RK_HEUR_ONES
        if (mode != RK_HEUR_ONES) {
            if (draw_vals) {
                x = draw_vals[(long long)r * F + k];
            } else {
                double mu = gmean, sd = gstd;
                if (mode == RK_HEUR_ITEM && (unsigned)c < (unsigned)n_items && item_count[c] > 0) mu = sd = item_mean[c];
                x = mu + sd * std_normal(rk_draw_key(seed, stream, r, 0x1000 + k), rk_draw_key(seed, stream, r, 0x2000 + k));
            }
            x = fmin(fmax(rint(x), 1.0), 5.0);                   // np.round (half to even), then clip to [1, 5]
        }
        if ((unsigned)c < (unsigned)n_items) o[c] = (float)x;
    }
    if (t == 0 && rate > 0 && r < rate * a.n_targets) o[a.targets[r / rate]] = 5.0f;
    for (int s = t; s < a.n_sel; s += kBlock) o[a.selected[s]] = 5.0f;
}

}  // namespace

RK_EXPORT int rk_heur_item_stats(int32_t n_items, int64_t nnz, const int32_t *col, const float *val, int32_t *item_count, double *item_mean,
                                 double *global, int32_t *n_rated, void *stream)
{
    if (n_items <= 0 || nnz < 0 || (nnz > 0 && (!col || !val)) || !item_count || !item_mean || !global || !n_rated)
        RK_FAIL(RK_EINVAL, "rk_heur_item_stats: bad arguments (n_items %d, nnz %lld)", n_items, (long long)nnz);
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)std::min<long long>(kMaxPartials, std::max<long long>(1, (nnz + kBlock - 1) / kBlock));
    RkScratch scratch(s);
    double *partial = nullptr;
    RK_HIP(scratch.get(&partial, (size_t)grid));
    RK_HIP(rk_zero_async(item_count, sizeof(int32_t) * (size_t)n_items, s));
    RK_HIP(rk_zero_async(item_mean, sizeof(double) * (size_t)n_items, s));
    RK_HIP(rk_zero_async(n_rated, sizeof(int32_t), s));
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(stats_pass_kernel, dim3(grid), dim3(kBlock), 0, s, pass, (long long)nnz, n_items, col, val, item_count, item_mean,
                           (const double *)global, partial);
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(stats_global_kernel, dim3(1), dim3(kBlock), 0, s, pass, grid, (long long)nnz, (const double *)partial, global);
        RK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stats_item_kernel, dim3((n_items + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n_items, (const int *)item_count,
                       item_mean, n_rated);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_heur_popular(int32_t n_items, const int32_t *item_count, int32_t k, int32_t *ids, int32_t *counts, int32_t *n_found,
                              void *stream)
{
    if (n_items <= 0 || k <= 0 || !item_count || !ids || !counts || !n_found)
        RK_FAIL(RK_EINVAL, "rk_heur_popular: bad arguments (n_items %d, k %d)", n_items, k);
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *keys = nullptr, *sorted = nullptr;
    int *n_d = nullptr;
    void *tmp = nullptr;
    size_t tb = 0;
    RK_HIP(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, tb, keys, sorted, n_items, 0, 64, s));
    RK_HIP(scratch.get(&keys, (size_t)n_items));
    RK_HIP(scratch.get(&sorted, (size_t)n_items));
    RK_HIP(scratch.get(&n_d, 1));
    RK_HIP(scratch.bytes(&tmp, tb));
    RK_HIP(rk_zero_async(n_d, sizeof(int), s));
    hipLaunchKernelGGL(popular_keys_kernel, dim3((n_items + 255) / 256), dim3(256), 0, s, n_items, item_count, keys);
    RK_CHECK_LAUNCH();
    RK_HIP(hipcub::DeviceRadixSort::SortKeysDescending(tmp, tb, keys, sorted, n_items, 0, 64, s));
    hipLaunchKernelGGL(popular_take_kernel, dim3((k + 255) / 256), dim3(256), 0, s, n_items, k, (const unsigned long long *)sorted, ids,
                       counts, n_d);
    RK_CHECK_LAUNCH();
    RK_HIP(hipMemcpyAsync(n_found, n_d, sizeof(int), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    return RK_OK;
}

RK_EXPORT int rk_heur_generate(int32_t attack_num, int32_t n_items, int32_t filler_num, const int32_t *targets, int32_t n_targets,
                               const int32_t *selected, int32_t n_sel, int32_t mode, double global_mean, double global_std,
                               const double *item_mean, const int32_t *item_count, const int32_t *draw_cols, const double *draw_vals,
                               uint64_t seed, uint64_t stream_id, float *out, void *stream)
{
    if (attack_num <= 0 || n_items <= 0 || !out || !targets || (n_sel > 0 && !selected))
        RK_FAIL(RK_EINVAL, "rk_heur_generate: bad arguments (attack_num %d, n_items %d)", attack_num, n_items);
    if (filler_num <= 0 || filler_num > RK_HEUR_MAX_FILLER || n_targets <= 0 || n_targets > RK_HEUR_MAX_TARGETS || n_sel < 0 ||
        n_sel > RK_HEUR_MAX_SELECT)
        RK_FAIL(RK_EINVAL, "rk_heur_generate: filler_num %d (1..%d), %d targets (1..%d), %d selected ids (0..%d)", filler_num,
                RK_HEUR_MAX_FILLER, n_targets, RK_HEUR_MAX_TARGETS, n_sel, RK_HEUR_MAX_SELECT);
    if (mode != RK_HEUR_GLOBAL && mode != RK_HEUR_ITEM && mode != RK_HEUR_ONES) RK_FAIL(RK_EINVAL, "rk_heur_generate: mode %d", mode);
    if ((draw_vals && !draw_cols) || (draw_cols && mode != RK_HEUR_ONES && !draw_vals))
        RK_FAIL(RK_EINVAL, "rk_heur_generate: the replay form takes draw_cols, and draw_vals with them unless the mode is ONES");
    if (!draw_cols && mode != RK_HEUR_ONES && !(std::isfinite(global_mean) && std::isfinite(global_std) && global_std >= 0.0))
        RK_FAIL(RK_EINVAL, "rk_heur_generate: global mean %g / std %g", global_mean, global_std);
    if (!draw_cols && mode == RK_HEUR_ITEM && (!item_mean || !item_count))
        RK_FAIL(RK_EINVAL, "rk_heur_generate: the ITEM mode needs item_mean and item_count");
    HeurSets a{};
    a.n_targets = n_targets;
    a.n_sel = n_sel;
    for (int k = 0; k < n_targets + n_sel; ++k) {
        const int id = k < n_targets ? targets[k] : selected[k - n_targets];
        if (id < 0 || id >= n_items) RK_FAIL(RK_EINVAL, "rk_heur_generate: item id %d outside [0, %d)", id, n_items);
        (k < n_targets ? a.targets[k] : a.selected[k - n_targets]) = id;
        a.excl[k] = id;
    }
    std::sort(a.excl, a.excl + n_targets + n_sel);
    a.n_excl = (int)(std::unique(a.excl, a.excl + n_targets + n_sel) - a.excl);
    if (n_items - a.n_excl < filler_num)
        RK_FAIL(RK_EINVAL, "rk_heur_generate: filler_num %d above the pool of %d items outside the targets and selected ids", filler_num,
                n_items - a.n_excl);
    hipLaunchKernelGGL(generate_kernel, dim3(attack_num), dim3(kBlock), 0, (hipStream_t)stream, n_items, filler_num, attack_num / n_targets, a,
                       mode, global_mean, global_std, item_mean, item_count, draw_cols, draw_vals, (unsigned long long)seed,
                       (unsigned long long)stream_id, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
