// SLIM victim (Ning and Karypis 2011): sparse non-negative item-item weights with a zero diagonal, one elastic-net regression per
// item, fitted by cyclic coordinate descent on G = X^T X + beta I (what rk_ease_gram writes).  include/recad_hip.h states the
// definition.  One workgroup per column j keeps the residual r and the weights w of its column in LDS.  The chain of coordinates is
// sequential, so the workgroup walks it 256 coordinates at a time: every thread works out the step of its own coordinate from the
// current r, the lowest coordinate whose step changes its weight is applied (row k of G read as coalesced lines, the I-wide update
// of r spread over the workgroup), and the coordinates after it are worked out again, since r moved.  A coordinate whose step is
// zero leaves the state as it was, so passing over it is the sequential order.  Thread t owns the elements i = t mod 256 of r and
// w in every loop, the coordinate it works out included, so the arrays need no barrier: the one barrier of a round is the agreement.  The only wide operation is elementwise: nothing
// is reduced in floating point and nothing adds floats atomically, so the result is the definition's to the bit.
#include <limits.h>
#include <math.h>

#include "common.h"

static constexpr int kSlThreads = 256;
static constexpr int kSlWaves = kSlThreads / 64;
static constexpr int kSlBatch = 16;                             // strides of the I-wide update whose loads of row k are issued together
static constexpr int kSlScratchBytes = 64;                      // two parities of {delta, lane} per wave
static_assert(2 * kSlWaves * (sizeof(float) + sizeof(int)) == kSlScratchBytes, "the scratch behind r and w");
static_assert(8LL * RK_SLIM_MAX_ITEMS + kSlScratchBytes <= kLdsMaxBytes - 64, "RK_SLIM_MAX_ITEMS does not fit a CU's LDS");
static_assert(8LL * (RK_SLIM_MAX_ITEMS + 1) + kSlScratchBytes > kLdsMaxBytes - 64, "RK_SLIM_MAX_ITEMS is not the largest catalogue");

// status[1] <- the lowest k whose G_kk is not a finite number > 0
__global__ __launch_bounds__(256) void slim_diag_check_kernel(int n, const float *__restrict__ G, int *__restrict__ status)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float g = G[(size_t)k * n + k];
    if (!(g > 0.0f) || !isfinite(g)) atomicMin(status + 1, k);
}

// One coordinate step from (r_k, w_k): the new weight, and delta = fl(w' - w_k).  Every operation is rounded on its own.
__device__ __forceinline__ float sl_step(float rk, float wk, float l1, float gkk, float *w_new)
{
#pragma clang fp contract(off)
    const float t = rk - l1;
    const float q = t / gkk;
    const float v = wk + q;
    const float wn = v > 0.0f ? v : 0.0f;
    *w_new = wn;
    return wn - wk;
}

// r - fl(delta * g): two roundings, never one fused multiply-add
__device__ __forceinline__ float sl_sub_term(float r, float delta, float g)
{
#pragma clang fp contract(off)
    const float term = delta * g;
    return r - term;
}

__global__ __launch_bounds__(kSlThreads) void slim_fit_kernel(int n, const float *__restrict__ G, float l1, int sweeps, float *__restrict__ W,
                                                              int *__restrict__ info, float *__restrict__ R_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_lds[];
    float *r = reinterpret_cast<float *>(sl_lds), *w = r + n;
    float *sdel = w + n;                                        // [2][kSlWaves]: the step of each wave's lowest changing coordinate
    int *slane = reinterpret_cast<int *>(sdel + 2 * kSlWaves);  // [2][kSlWaves]: its lane, 64 when the wave has none
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = blockIdx.x;
    for (int i = tid; i < n; i += kSlThreads) {
        r[i] = G[(size_t)i * n + j];
        w[i] = 0.0f;
    }
    __syncthreads();
    int last = 0, steps = 0, par = 0;
#pragma unroll 1
    for (int s = 1; s <= sweeps; ++s) {
        bool changed = false;
#pragma unroll 1
        for (int k0 = 0; k0 < n; k0 += kSlThreads) {
            const int k = k0 + tid;
            const bool mine = k < n && k != j;
            float gkk = 1.0f;
            bool have = false;
            int lo = 0;                                         // coordinates below k0 + lo have had their turn in this sweep
#pragma unroll 1
            for (int it = 0; it < kSlThreads; ++it) {           // each round applies one coordinate and lo passes it: at most 256
                float delta = 0.0f, w_new = 0.0f;
                if (mine && tid >= lo) {
                    const float wk = w[k], rk = r[k];
                    if (wk != 0.0f || rk > l1) {                // otherwise v = fl(0 + q) with q <= 0: the step is zero
                        if (!have) {
                            gkk = G[(size_t)k * n + k];
                            have = true;
                        }
                        delta = sl_step(rk, wk, l1, gkk, &w_new);
                    }
                }
                const unsigned long long b = __ballot(delta != 0.0f);
                const int first = b ? __ffsll((long long)b) - 1 : 64;
                if (lane == first) sdel[par * kSlWaves + wave] = delta;
                if (lane == 0) slane[par * kSlWaves + wave] = first;
                __syncthreads();
                int cw = -1, cl = 64;
#pragma unroll
                for (int q = kSlWaves - 1; q >= 0; --q) {
                    const int l = slane[par * kSlWaves + q];
                    if (l < 64) {
                        cw = q;
                        cl = l;
                    }
                }
                if (cw < 0) {                                   // the same in every thread: nothing in the rest of the block changes
                    par ^= 1;
                    break;
                }
                const int c = cw * 64 + cl;
                const float d = sdel[par * kSlWaves + cw];
                par ^= 1;                                       // the next round writes the other half: this one may still be read,
                                                                // and the round after it lies behind the next round's barrier
                if (tid == c) w[k] = w_new;
                const float *__restrict__ row = G + (size_t)(k0 + c) * n;
                // the step waits for row k once, not once per stride: kSlBatch loads are in flight before the first is used
#pragma unroll 1
                for (int i0 = tid; i0 < n; i0 += kSlThreads * kSlBatch) {
                    float g[kSlBatch];
#pragma unroll
                    for (int b = 0; b < kSlBatch; ++b) {
                        const int i = i0 + b * kSlThreads;
                        g[b] = i < n ? row[i] : 0.0f;
                    }
#pragma unroll
                    for (int b = 0; b < kSlBatch; ++b) {
                        const int i = i0 + b * kSlThreads;
                        if (i < n) r[i] = sl_sub_term(r[i], d, g[b]);
                    }
                }
                ++steps;
                changed = true;
                lo = c + 1;                                     // no barrier here: r[i] and w[i] with i = tid mod 256 are this thread's alone
            }
        }
        if (!changed) break;                                    // a sweep that changes nothing leaves every later sweep nothing to change
        last = s;
    }
    __syncthreads();
    int positive = 0;
    for (int i = tid; i < n; i += kSlThreads) {
        const float wi = w[i];
        W[(size_t)i * n + j] = wi;
        if (R_out) R_out[(size_t)i * n + j] = r[i];
        positive += wi > 0.0f ? 1 : 0;
    }
    if (info) {
        positive = block_sum_256(positive, slane);
        if (tid == 0) {
            info[3 * j + 0] = last;
            info[3 * j + 1] = positive;
            info[3 * j + 2] = steps;
        }
    }
}

RK_EXPORT int rk_slim_fit(int32_t n_items, const float *G, float l1, int32_t sweeps, float *W, int32_t *info, float *R_out, int32_t *status,
                          void *stream)
{
    if (!G || !W || !status) RK_FAIL(RK_EINVAL, "rk_slim_fit: bad arguments");
    if (n_items < 1 || n_items > RK_SLIM_MAX_ITEMS)
        RK_FAIL(RK_EINVAL, "rk_slim_fit: %d items outside 1..%d (r and w of a column live in one workgroup's LDS)", n_items, RK_SLIM_MAX_ITEMS);
    if (sweeps < 1) RK_FAIL(RK_EINVAL, "rk_slim_fit: sweeps = %d, at least 1", sweeps);
    if (!isfinite(l1) || !(l1 >= 0.0f)) RK_FAIL(RK_EINVAL, "rk_slim_fit: l1 = %g is not a finite number >= 0", (double)l1);
    hipStream_t s = (hipStream_t)stream;
    int st[2] = {0, INT_MAX};
    RK_HIP(rk_set_status(status, 0, INT_MAX, s));
    hipLaunchKernelGGL(slim_diag_check_kernel, dim3((n_items + 255) / 256), dim3(256), 0, s, n_items, G, status);
    RK_CHECK_LAUNCH();
    RK_HIP(hipMemcpyAsync(st, status, sizeof(st), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    const bool bad = st[1] != INT_MAX;
    RK_HIP(rk_set_status(status, bad ? RK_SLIM_BAD_DIAG : 0, bad ? st[1] : -1, s));
    if (bad) RK_FAIL(RK_EINVAL, "rk_slim_fit: diagonal entry %d is not a finite positive number", st[1]);
    static RkPerDeviceOnce attr_once;
    int attr_dev;
    if (attr_once.need(&attr_dev)) {
        RK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(slim_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxBytes - 64));
        attr_once.done(attr_dev);
    }
    const size_t lds = (size_t)8 * n_items + kSlScratchBytes;
    hipLaunchKernelGGL(slim_fit_kernel, dim3(n_items), dim3(kSlThreads), lds, s, n_items, G, l1, sweeps, W, info, R_out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
