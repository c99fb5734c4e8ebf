// PGA attacker (Li, Wang, Singh and Vorobeychik 2016): projected gradient ascent on the fake profiles through one sweep of an
// iALS surrogate.  include/recad_hip.h states the definition.  rk_ials_solve_rhs is rk_ials_half_sweep with the right-hand side
// read from a buffer: the same device code (ials_solve.h) builds and factorises A_u.  rk_pga_loss turns a block of score rows
// into the loss terms and D, one wave per row, lse and softmax in double.  rk_pga_user_adjoint, rk_pga_grad and rk_pga_step are
// the adjoint of the fake rows, the A x I gradient with its largest magnitude, and the projected step with the per-row selection.
// Nothing here adds floats atomically: every float sum has one owner and a fixed order; the only atomics are on integers.
#include "ials_solve.h"

static constexpr int kPgThreads = 256;
static constexpr int kPgRowTile = 8;                              // fake rows held in LDS by one workgroup of rk_pga_grad
static constexpr int kPgEntryChunk = 256;                         // entries of a fake row whose dots rk_pga_user_adjoint holds at once
static_assert(RK_PGA_MAX_TARGETS <= kPgThreads, "one thread pins one target");

// ---------------------------------------------------------------------------------------------------- rk_ials_solve_rhs
template <int NT>
__global__ __launch_bounds__(kIaThreads) void ials_solve_rhs_kernel(int n_rows, int n_cols, int d, const float *__restrict__ G,
                                                                    const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                    const float *__restrict__ val, float alpha,
                                                                    const float *__restrict__ Y, const float *__restrict__ rhs,
                                                                    const int *__restrict__ order, float *__restrict__ X,
                                                                    int *__restrict__ status)
{
    extern __shared__ float ia_lds[];
    constexpr int dp = 16 * NT;
    const int u = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)u >= (unsigned)n_rows) return;
    const IaLds l = ia_carve(ia_lds, dp, true);
    ia_build_system<NT>(l, n_cols, d, G, col, val, rowptr[u], rowptr[u + 1], alpha, Y);
    if ((int)threadIdx.x < dp) l.b[threadIdx.x] = (int)threadIdx.x < d ? rhs[(size_t)u * d + threadIdx.x] : 0.0f;   // b_u gives way
    __syncthreads();
    if (!ia_cholesky(d, ia_lda(dp), l.A)) {
        if (threadIdx.x == 0) {
            atomicMin(reinterpret_cast<unsigned *>(status) + 1, (unsigned)u);
            atomicExch(status, RK_IALS_NOT_SPD);
        }
        return;
    }
    ia_solve(d, ia_lda(dp), l.A, l.b, X + (size_t)u * d);
}

static hipError_t pg_allow_lds()
{
    static RkPerDeviceOnce once;
    int dev;
    if (!once.need(&dev)) return hipSuccess;
#define PG_ATTR(NT)                                                                                                     \
    do {                                                                                                                \
        hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(ials_solve_rhs_kernel<NT>),                  \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxBytes - 64);             \
        if (e_ != hipSuccess) return e_;                                                                                \
    } while (0)
    PG_ATTR(1); PG_ATTR(2); PG_ATTR(3); PG_ATTR(4); PG_ATTR(5); PG_ATTR(6); PG_ATTR(7); PG_ATTR(8);
#undef PG_ATTR
    once.done(dev);
    return hipSuccess;
}

RK_EXPORT int rk_ials_solve_rhs(int32_t n_rows, int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col,
                                const float *val, float alpha, const float *Y, const float *rhs, const int32_t *order, float *X_out,
                                int32_t *status, void *stream)
{
    if (n_rows < 1 || n_cols < 1 || !G || !rowptr || !col || !val || !Y || !rhs || !X_out || !status)
        RK_FAIL(RK_EINVAL, "rk_ials_solve_rhs: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_solve_rhs: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(alpha)) RK_FAIL(RK_EINVAL, "rk_ials_solve_rhs: alpha = %g is not a finite number >= 0", (double)alpha);
    RK_HIP(pg_allow_lds());
    hipStream_t s = (hipStream_t)stream;
    const int dp = ia_dp(d);
    const size_t lds = sizeof(float) * ia_lds_floats(dp, true);
    RK_HIP(rk_set_status(status, 0, -1, s));
#define IA_CALL(NT)                                                                                                                  \
    hipLaunchKernelGGL(ials_solve_rhs_kernel<NT>, dim3(n_rows), dim3(kIaThreads), lds, s, n_rows, n_cols, d, G, rowptr, col, val, alpha, Y, \
                       rhs, order, X_out, status)
    IA_DISPATCH(dp / 16, IA_CALL);
#undef IA_CALL
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---------------------------------------------------------------------------------------------------- rk_pga_loss
template <typename T>
__device__ __forceinline__ T pg_wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// One wave per row of the block.  The row's rated items are marked -inf in place (the wave owns its row; the barrier orders the
// marks before the reads), then three passes: the largest score, the sum of exp in double, D.  No __restrict__ on S: it is read
// and written.
__global__ __launch_bounds__(kPgThreads) void pga_loss_kernel(int nb, int n_items, float *S, const int *__restrict__ rowptr,
                                                              const int *__restrict__ col, int user0, int target,
                                                              const int *__restrict__ eligible, double inv_count,
                                                              double *__restrict__ terms)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (kPgThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool valid = row < nb;
    const int u = user0 + row;
    const bool elig = valid && eligible[u] != 0;
    float *s = S + (size_t)(valid ? row : 0) * n_items;
    if (elig) {
        const int end = rowptr[u + 1];
        for (int e = rowptr[u] + lane; e < end; e += 64) {
            const int c = col[e];
            if ((unsigned)c < (unsigned)n_items) s[c] = -INFINITY;
        }
    }
    __syncthreads();
    if (!valid) return;
    if (!elig) {
        for (int j = lane; j < n_items; j += 64) s[j] = 0.0f;
        if (lane == 0) terms[row] = 0.0;
        return;
    }
    float m = -INFINITY;
    for (int j = lane; j < n_items; j += 64) m = fmaxf(m, s[j]);
    m = pg_wave_max(m);
    double sum = 0.0;
    for (int j = lane; j < n_items; j += 64) {
        const float v = s[j];
        if (v != -INFINITY) sum += exp((double)v - (double)m);
    }
    sum = wave_sum(sum);
    const double lse = (double)m + log(sum);
    const double st = (double)s[target];                           // read by every lane before any lane overwrites it
    for (int j = lane; j < n_items; j += 64) {
        const float v = s[j];
        float dj = 0.0f;
        if (v != -INFINITY) dj = (float)((exp((double)v - lse) - (j == target ? 1.0 : 0.0)) * inv_count);
        s[j] = dj;
    }
    if (lane == 0) terms[row] = (lse - st) * inv_count;
}

RK_EXPORT int rk_pga_loss(int32_t nb, int32_t n_items, float *scores, const int32_t *rowptr, const int32_t *col, int32_t user0,
                          int32_t target, const int32_t *eligible, double inv_count, double *terms, void *stream)
{
    if (nb < 1 || n_items < 1 || user0 < 0 || !scores || !rowptr || !col || !eligible || !terms)
        RK_FAIL(RK_EINVAL, "rk_pga_loss: bad arguments");
    if (target < 0 || target >= n_items) RK_FAIL(RK_EINVAL, "rk_pga_loss: target %d outside [0, %d)", target, n_items);
    if (!isfinite(inv_count) || !(inv_count > 0.0)) RK_FAIL(RK_EINVAL, "rk_pga_loss: inv_count = %g is not a finite positive number", inv_count);
    const int rows = kPgThreads / 64;
    hipLaunchKernelGGL(pga_loss_kernel, dim3((nb + rows - 1) / rows), dim3(kPgThreads), 0, (hipStream_t)stream, nb, n_items, scores, rowptr,
                       col, user0, target, eligible, inv_count, terms);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// out[0] = the n doubles: thread t sums terms t, t + 256, ... in order, the threads by block_sum_256
__global__ __launch_bounds__(kPgThreads) void pga_loss_sum_kernel(long long n, const double *__restrict__ terms, double *__restrict__ out)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n; i += kPgThreads) acc += terms[i];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[0] = acc;
}

RK_EXPORT int rk_pga_loss_sum(int64_t n, const double *terms, double *out, void *stream)
{
    if (n < 1 || !terms || !out) RK_FAIL(RK_EINVAL, "rk_pga_loss_sum: bad arguments");
    hipLaunchKernelGGL(pga_loss_sum_kernel, dim3(1), dim3(kPgThreads), 0, (hipStream_t)stream, (long long)n, terms, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// out[i] = (((p_0 + p_1) + p_2) + ...)[i]: the blocks' partial products in block order
__global__ __launch_bounds__(kPgThreads) void pga_add_blocks_kernel(long long n, int n_parts, const float *__restrict__ parts, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * kPgThreads + threadIdx.x;
    if (i >= n) return;
    float s = parts[i];
    for (int p = 1; p < n_parts; ++p) s = s + parts[(size_t)p * n + i];
    out[i] = s;
}

RK_EXPORT int rk_pga_add_blocks(int64_t n, int32_t n_parts, const float *parts, float *out, void *stream)
{
    if (n < 1 || n_parts < 1 || n > (int64_t)INT_MAX * kPgThreads || !parts || !out) RK_FAIL(RK_EINVAL, "rk_pga_add_blocks: bad arguments");
    hipLaunchKernelGGL(pga_add_blocks_kernel, dim3((unsigned)((n + kPgThreads - 1) / kPgThreads)), dim3(kPgThreads), 0, (hipStream_t)stream,
                       (long long)n, n_parts, parts, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---------------------------------------------------------------------------------------------------- rk_pga_user_adjoint
// One workgroup per fake row.  Per chunk of entries the four waves compute s+_e = x . y+_j and q_e = x . z_j (lanes over k, the
// butterfly sum) and from them cf_e = 1 + wbar (1 - s+_e) and wq_e = wbar q_e; then thread k < d adds the chunk's entries in column
// order, t_k += fl(fl(cf_e z_jk) - fl(wq_e y+_jk)).  (1 + wbar) z - wbar s+ z is written as cf z: s+ is near 1 on a fitted entry,
// and the two terms of the first form cancel to one part in wbar.
__global__ __launch_bounds__(kPgThreads) void pga_user_adjoint_kernel(int n_items, int d, const float *__restrict__ Z,
                                                                      const float *__restrict__ Yp, const float *__restrict__ Xf,
                                                                      const float *__restrict__ M, const int *__restrict__ fptr,
                                                                      const int *__restrict__ fcol, float wbar, float *__restrict__ H)
{
    __shared__ float x[RK_IALS_MAX_DIM], cf[kPgEntryChunk], wq[kPgEntryChunk];
    __shared__ int cols[kPgEntryChunk];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = blockIdx.x;
    if (tid < d) x[tid] = Xf[(size_t)f * d + tid];
    float t = 0.0f;
    const int beg = fptr[f], end = fptr[f + 1];
#pragma unroll 1
    for (int e0 = beg; e0 < end; e0 += kPgEntryChunk) {
        const int cnt = min(kPgEntryChunk, end - e0);
        __syncthreads();                                           // x is staged; the chunk before this one has been consumed
        for (int e = wave; e < cnt; e += kPgThreads / 64) {
            const int j = fcol[e0 + e];
            const bool ok = (unsigned)j < (unsigned)n_items;       // the wave's own entry: uniform
            float a = 0.0f, b = 0.0f;
            if (ok)
                for (int k = lane; k < d; k += 64) {
                    a = fmaf(x[k], Yp[(size_t)j * d + k], a);
                    b = fmaf(x[k], Z[(size_t)j * d + k], b);
                }
            a = wave_sum(a);
            b = wave_sum(b);
            if (lane == 0) {
#pragma clang fp contract(off)
                const float gap = 1.0f - a;                        // the fitted entry's residual first: no cancellation against wbar
                const float wg = wbar * gap;
                cf[e] = 1.0f + wg;
                wq[e] = wbar * b;
                cols[e] = ok ? j : -1;
            }
        }
        __syncthreads();
        if (tid < d) {
#pragma clang fp contract(off)
            for (int e = 0; e < cnt; ++e) {
                const int j = cols[e];
                if (j < 0) continue;
                const float u1 = cf[e] * Z[(size_t)j * d + tid], u2 = wq[e] * Yp[(size_t)j * d + tid];
                const float uu = u1 - u2;
                t = t + uu;
            }
        }
    }
    __syncthreads();                                               // x is staged (a row without entries)
    if (tid < d) {
#pragma clang fp contract(off)
        float m = 0.0f;
        for (int l = 0; l < d; ++l) {
            const float sym = M[tid * d + l] + M[l * d + tid];
            const float prod = sym * x[l];
            m = m + prod;
        }
        H[(size_t)f * d + tid] = t - m;
    }
}

RK_EXPORT int rk_pga_user_adjoint(int32_t n_fake, int32_t n_items, int32_t d, const float *Z, const float *Yp, const float *Xf,
                                  const float *M, const int32_t *fptr, const int32_t *fcol, float wbar, float *H, void *stream)
{
    if (n_fake < 1 || n_items < 1 || !Z || !Yp || !Xf || !M || !fptr || !fcol || !H) RK_FAIL(RK_EINVAL, "rk_pga_user_adjoint: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_pga_user_adjoint: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(wbar)) RK_FAIL(RK_EINVAL, "rk_pga_user_adjoint: wbar = %g is not a finite number >= 0", (double)wbar);
    hipLaunchKernelGGL(pga_user_adjoint_kernel, dim3(n_fake), dim3(kPgThreads), 0, (hipStream_t)stream, n_items, d, Z, Yp, Xf, M, fptr, fcol,
                       wbar, H);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---------------------------------------------------------------------------------------------------- rk_pga_grad
__global__ void pga_zero_word_kernel(unsigned *w) { w[0] = 0u; }

// Workgroup (bx, by): items [256 bx, 256 bx + 256), fake rows [8 by, 8 by + 8).  The rows' x_f and v_f sit in LDS; thread j walks
// its item's three table rows once and keeps four k-ordered fmaf chains per fake row.  The largest |grad| of the workgroup goes
// into gmax by an integer max on the bit pattern (order-free, so the same bits every run).
__global__ __launch_bounds__(kPgThreads) void pga_grad_kernel(int n_fake, int n_items, int d, const float *__restrict__ Xf,
                                                              const float *__restrict__ V, const float *__restrict__ Z,
                                                              const float *__restrict__ Yp, const float *__restrict__ Yo, float wbar,
                                                              float *__restrict__ grad, unsigned *__restrict__ gmax)
{
    __shared__ float xs[kPgRowTile][RK_IALS_MAX_DIM], vs[kPgRowTile][RK_IALS_MAX_DIM];
    __shared__ unsigned red[kPgThreads / 64];
    const int tid = threadIdx.x;
    const int f0 = blockIdx.y * kPgRowTile, nf = min(kPgRowTile, n_fake - f0);
    for (int at = tid; at < kPgRowTile * d; at += kPgThreads) {
        const int r = at / d, k = at - r * d;
        xs[r][k] = r < nf ? Xf[(size_t)(f0 + r) * d + k] : 0.0f;
        vs[r][k] = r < nf ? V[(size_t)(f0 + r) * d + k] : 0.0f;
    }
    __syncthreads();
    const int j = blockIdx.x * kPgThreads + tid;
    unsigned mx = 0u;
    if (j < n_items) {
        float a[kPgRowTile], sp[kPgRowTile], so[kPgRowTile], b[kPgRowTile];
#pragma unroll
        for (int r = 0; r < kPgRowTile; ++r) a[r] = sp[r] = so[r] = b[r] = 0.0f;
        const float *zr = Z + (size_t)j * d, *pr = Yp + (size_t)j * d, *orow = Yo + (size_t)j * d;
#pragma unroll 1
        for (int k = 0; k < d; ++k) {
            const float z = zr[k], yp = pr[k], yo = orow[k];
#pragma unroll
            for (int r = 0; r < kPgRowTile; ++r) {
                const float x = xs[r][k], v = vs[r][k];
                a[r] = fmaf(x, z, a[r]);
                sp[r] = fmaf(x, yp, sp[r]);
                so[r] = fmaf(x, yo, so[r]);
                b[r] = fmaf(yo, v, b[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kPgRowTile; ++r) {
            if (r >= nf) break;
            // 1 + wbar - wbar s as 1 + wbar (1 - s): s is near 1 on a fitted entry (see rk_pga_user_adjoint)
            const float g = (1.0f + wbar * (1.0f - sp[r])) * a[r] + (1.0f + wbar * (1.0f - so[r])) * b[r];
            grad[(size_t)(f0 + r) * n_items + j] = g;
            const unsigned bits = __float_as_uint(fabsf(g));
            mx = bits > mx ? bits : mx;
        }
    }
    mx = pg_wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        unsigned m = red[0];
        for (int w = 1; w < kPgThreads / 64; ++w) m = red[w] > m ? red[w] : m;
        if (m) atomicMax(gmax, m);
    }
}

RK_EXPORT int rk_pga_grad(int32_t n_fake, int32_t n_items, int32_t d, const float *Xf, const float *V, const float *Z, const float *Yp,
                          const float *Yo, float wbar, float *grad, uint32_t *gmax, void *stream)
{
    if (n_fake < 1 || n_items < 1 || !Xf || !V || !Z || !Yp || !Yo || !grad || !gmax) RK_FAIL(RK_EINVAL, "rk_pga_grad: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_pga_grad: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(wbar)) RK_FAIL(RK_EINVAL, "rk_pga_grad: wbar = %g is not a finite number >= 0", (double)wbar);
    const int by = (n_fake + kPgRowTile - 1) / kPgRowTile;
    if (by > 65535) RK_FAIL(RK_EINVAL, "rk_pga_grad: %d fake rows, at most %d", n_fake, 65535 * kPgRowTile);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pga_zero_word_kernel, dim3(1), dim3(1), 0, s, gmax);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(pga_grad_kernel, dim3((n_items + kPgThreads - 1) / kPgThreads, by), dim3(kPgThreads), 0, s, n_fake, n_items, d, Xf, V, Z,
                       Yp, Yo, wbar, grad, gmax);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

// ---------------------------------------------------------------------------------------------------- rk_pga_step
// sum over the block of a 0 / 1 flag, and the number of set flags in threads before this one: ballots inside a wave, the four
// waves' counts through tot ([4], LDS).  The caller separates two uses of one tot by a barrier.
__device__ __forceinline__ int pg_block_rank(bool flag, int *tot, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) tot[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ULL << lane) - 1ULL)), all = 0;
    for (int w = 0; w < kPgThreads / 64; ++w) {
        if (w < wave) before += tot[w];
        all += tot[w];
    }
    *total = all;
    return before;
}

// One workgroup per fake row: the update and the pinning, a radix select (four passes of eight bits over the bit patterns, which
// order non-negative floats) for the filler_num-th largest non-target strength T, then an ordered compaction over the row: the
// targets, everything above T, and the lowest ids among the entries equal to T, written in ascending column order.
__global__ __launch_bounds__(kPgThreads) void pga_step_kernel(int n_items, float *R, const float *__restrict__ grad,
                                                              const unsigned *__restrict__ gmax, float lr, int n_targets,
                                                              const int *__restrict__ targets, int filler_num, int *__restrict__ fcol)
{
    __shared__ int tg[RK_PGA_MAX_TARGETS];
    __shared__ int hist[256];
    __shared__ unsigned sel_prefix;
    __shared__ int sel_need;
    __shared__ int tot_eq[kPgThreads / 64], tot_sel[kPgThreads / 64];
    const int tid = threadIdx.x;
    const int f = blockIdx.x;
    float *r = R + (size_t)f * n_items;
    if (tid < n_targets) tg[tid] = targets[tid];
    __syncthreads();
    const unsigned gbits = grad ? gmax[0] : 0u;
    if (gbits) {
#pragma clang fp contract(off)
        const float gm = __uint_as_float(gbits);
        const float *g = grad + (size_t)f * n_items;
        for (int j = tid; j < n_items; j += kPgThreads) {
            const float qn = g[j] / gm;
            const float st = lr * qn;
            const float v = r[j] - st;
            r[j] = v > 0.0f ? fminf(v, 1.0f) : 0.0f;               // a NaN, a negative number and -0.0f all become +0.0f
        }
    }
    __syncthreads();                                               // the update is done before the targets are pinned
    if (tid < n_targets && (unsigned)tg[tid] < (unsigned)n_items) r[tg[tid]] = 1.0f;
    __syncthreads();

    auto is_target = [&](int j) {
        bool t = false;
        for (int i = 0; i < n_targets; ++i) t |= tg[i] == j;
        return t;
    };
    unsigned T = 0xFFFFFFFFu;                                       // filler_num = 0: nothing is above or equal
    int need = 0;
    if (filler_num > 0) {
        if (tid == 0) {
            sel_prefix = 0u;
            sel_need = filler_num;
        }
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const unsigned prefix = sel_prefix;
            for (int j = tid; j < n_items; j += kPgThreads) {
                if (is_target(j)) continue;
                const unsigned key = __float_as_uint(r[j]);
                if (shift == 24 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int left = sel_need, b = 255;
                while (b > 0 && hist[b] < left) left -= hist[b--];
                sel_prefix = (prefix << 8) | (unsigned)b;
                sel_need = left;
            }
            __syncthreads();
        }
        T = sel_prefix;
        need = sel_need;
    }
    const int len = n_targets + filler_num;
    int *out = fcol + (size_t)f * len;
    int base_eq = 0, base_out = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < n_items; j0 += kPgThreads) {
        const int j = j0 + tid;
        const bool valid = j < n_items;
        const bool tgt = valid && is_target(j);
        const unsigned key = valid ? __float_as_uint(r[j]) : 0u;
        const bool eq = valid && !tgt && key == T, gt = valid && !tgt && key > T;
        int n_eq, n_sel;
        const int eq_rank = base_eq + pg_block_rank(eq, tot_eq, &n_eq);
        const bool sel = tgt || gt || (eq && eq_rank < need);
        const int pos = base_out + pg_block_rank(sel, tot_sel, &n_sel);
        if (sel && pos < len) out[pos] = j;
        base_eq += n_eq;
        base_out += n_sel;
    }
}

RK_EXPORT int rk_pga_step(int32_t n_fake, int32_t n_items, float *R, const float *grad, const uint32_t *gmax, float lr, int32_t n_targets,
                          const int32_t *targets, int32_t filler_num, int32_t *fcol_out, void *stream)
{
    if (n_fake < 1 || n_items < 1 || !R || !targets || !fcol_out || (grad && !gmax)) RK_FAIL(RK_EINVAL, "rk_pga_step: bad arguments");
    if (n_targets < 1 || n_targets > RK_PGA_MAX_TARGETS || n_targets > n_items)
        RK_FAIL(RK_EINVAL, "rk_pga_step: %d targets, expected 1..%d and at most the %d items", n_targets, RK_PGA_MAX_TARGETS, n_items);
    if (filler_num < 0 || filler_num > n_items - n_targets)
        RK_FAIL(RK_EINVAL, "rk_pga_step: filler_num = %d outside [0, %d] (the items that are no targets)", filler_num, n_items - n_targets);
    if (grad && (!isfinite(lr) || !(lr > 0.0f))) RK_FAIL(RK_EINVAL, "rk_pga_step: lr = %g is not a finite positive number", (double)lr);
    hipLaunchKernelGGL(pga_step_kernel, dim3(n_fake), dim3(kPgThreads), 0, (hipStream_t)stream, n_items, R, grad, gmax, lr, n_targets, targets,
                       filler_num, fcol_out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
