// iALS victim (Hu, Koren and Volinsky 2008): weighted matrix factorisation fitted by alternating least squares, one row's d x d
// system at a time.  include/recad_hip.h states the definition.  rk_ials_gram forms G = Y^T Y + lambda I from per-block partials
// on the fp32 MFMA.  rk_ials_half_sweep gives every row one workgroup: the row's entries are staged in LDS 64 at a time, the
// lower-triangle 16 x 16 tiles of sum_e w_e y y^T are accumulated with v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain),
// shared among the four waves, G is added, and A_u is factorised (Cholesky) and solved inside LDS.  rk_ials_system is the same
// device code up to the factorisation, written out.  rk_ials_gram64 and rk_ials_objective evaluate the objective in float64
// without the dense matrix.  Nothing here adds floats atomically: every sum has one owner and a fixed order.
#include "ials_solve.h"

template <int NT>
__global__ __launch_bounds__(kIaThreads) void ials_half_sweep_kernel(int n_rows, int n_cols, int d, const float *__restrict__ G,
                                                                     const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                     const float *__restrict__ val, float alpha,
                                                                     const float *__restrict__ Y, const int *__restrict__ order,
                                                                     float *__restrict__ X, int *__restrict__ status)
{
    extern __shared__ float ia_lds[];
    const int u = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)u >= (unsigned)n_rows) return;
    const IaLds l = ia_carve(ia_lds, 16 * NT, true);
    ia_build_system<NT>(l, n_cols, d, G, col, val, rowptr[u], rowptr[u + 1], alpha, Y);
    if (!ia_cholesky(d, ia_lda(16 * NT), l.A)) {
        if (threadIdx.x == 0) {
            atomicMin(reinterpret_cast<unsigned *>(status) + 1, (unsigned)u);
            atomicExch(status, RK_IALS_NOT_SPD);
        }
        return;
    }
    ia_solve(d, ia_lda(16 * NT), l.A, l.b, X + (size_t)u * d);
}

template <int NT>
__global__ __launch_bounds__(kIaThreads) void ials_system_kernel(int n_cols, int d, const float *__restrict__ G,
                                                                 const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                 const float *__restrict__ val, float alpha, const float *__restrict__ Y,
                                                                 const int *__restrict__ row_ids, float *__restrict__ A_out,
                                                                 float *__restrict__ b_out)
{
    extern __shared__ float ia_lds[];
    const int u = row_ids[blockIdx.x];
    const IaLds l = ia_carve(ia_lds, 16 * NT, true);
    ia_build_system<NT>(l, n_cols, d, G, col, val, rowptr[u], rowptr[u + 1], alpha, Y);
    const int lda = ia_lda(16 * NT);
    float *A = A_out + (size_t)blockIdx.x * d * d;
    for (int at = threadIdx.x; at < d * d; at += kIaThreads) {
        const int i = at / d, j = at - i * d;
        A[at] = j <= i ? l.A[i * lda + j] : l.A[j * lda + i];
    }
    if ((int)threadIdx.x < d) b_out[(size_t)blockIdx.x * d + threadIdx.x] = l.b[threadIdx.x];
}

// Block b: the lower-triangle tiles of sum over rows [b * 256, b * 256 + 256) of y y^T, one fmaf chain in row order, into
// work[b] ([dp * dp]).
template <int NT>
__global__ __launch_bounds__(kIaThreads) void ials_gram_partial_kernel(int n, int d, const float *__restrict__ Y, float *__restrict__ work)
{
    extern __shared__ float ia_lds[];
    constexpr int dp = 16 * NT;
    const int ldy = ia_ldy(dp);
    const IaLds l = ia_carve(ia_lds, dp, false);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lo = blockIdx.x * kIaGramRows, hi = min(n, lo + kIaGramRows);
    IaAcc<NT> t;
    t.init(wave);
#pragma unroll 1
    for (int r0 = lo; r0 < hi; r0 += kIaChunk) {
        const int cnt = min(kIaChunk, hi - r0), rows4 = (cnt + 3) & ~3;
        __syncthreads();
        if (tid < kIaChunk) {
            l.col[tid] = tid < cnt ? r0 + tid : -1;
            l.w[tid] = 1.0f;
        }
        __syncthreads();
        ia_stage_rows(l, d, dp, ldy, rows4, Y);
        __syncthreads();
        t.add_rows(l, ldy, rows4, lane);
    }
    float *out = work + (size_t)blockIdx.x * dp * dp;
#pragma unroll
    for (int s = 0; s < IaTiles<NT>::S; ++s) {
        if (t.ro[s] < 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(t.ro[s] + 4 * (lane >> 4) + r) * dp + t.co[s] + (lane & 15)] = t.acc[s][r];
    }
}

// G[k][l] = G[l][k] = the partials in block order, lambda added to the diagonal last; one thread per element of the lower triangle
__global__ __launch_bounds__(kIaThreads) void ials_gram_finish_kernel(int n_blocks, int d, int dp, const float *__restrict__ work, float lambda,
                                                                      float *__restrict__ G)
{
    const int at = blockIdx.x * kIaThreads + threadIdx.x;
    if (at >= d * d) return;
    const int k = at / d, l = at - k * d;
    if (l > k) return;
    float s = work[k * dp + l];
    for (int b = 1; b < n_blocks; ++b) s = s + work[(size_t)b * dp * dp + k * dp + l];
    if (k == l) s = s + lambda;
    G[k * d + l] = s;
    G[l * d + k] = s;
}

// ---- float64: the objective
// The float64 Gram matrix splits the rows into at most 1024 blocks of at least 32 rows: its partials are d * d doubles each.
static inline int ia_gram64_rows(int n) { return std::max(32, (n + 1023) / 1024); }

__global__ __launch_bounds__(kIaThreads) void ials_gram64_partial_kernel(int n, int d, int rows, const float *__restrict__ Y,
                                                                         double *__restrict__ part)
{
    const int lo = blockIdx.x * rows, hi = min(n, lo + rows);
    for (int at = threadIdx.x; at < d * d; at += kIaThreads) {
        const int k = at / d, l = at - k * d;
        if (l > k) continue;
        double s = 0.0;
        for (int r = lo; r < hi; ++r) s += (double)Y[(size_t)r * d + k] * (double)Y[(size_t)r * d + l];
        part[(size_t)blockIdx.x * d * d + at] = s;
    }
}

__global__ __launch_bounds__(kIaThreads) void ials_gram64_finish_kernel(int n_blocks, int d, const double *__restrict__ part, double *__restrict__ GY)
{
    const int at = blockIdx.x * kIaThreads + threadIdx.x;
    if (at >= d * d) return;
    const int k = at / d, l = at - k * d;
    if (l > k) return;
    double s = part[at];
    for (int b = 1; b < n_blocks; ++b) s += part[(size_t)b * d * d + at];
    GY[k * d + l] = s;
    GY[l * d + k] = s;
}

// partial[u] = x_u^T GY x_u + sum_e [c_e (1 - s_e)^2 - s_e^2] + lambda |x_u|^2; one workgroup per row, every sum in a fixed order
__global__ __launch_bounds__(kIaThreads) void ials_objective_kernel(int n_cols, int d, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                                    const float *__restrict__ val, float alpha, float lambda,
                                                                    const float *__restrict__ X, const float *__restrict__ Y,
                                                                    const double *__restrict__ GY, double *__restrict__ partial)
{
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = blockIdx.x;
    const float *x = X + (size_t)u * d;
    double acc = 0.0;
    for (int at = tid; at < d * d; at += kIaThreads) {
        const int k = at / d, l = at - k * d;
        acc += (double)x[k] * GY[at] * (double)x[l];
    }
    for (int k = tid; k < d; k += kIaThreads) acc += (double)lambda * ((double)x[k] * (double)x[k]);
    const int end = rowptr[u + 1];
    for (int e = rowptr[u] + wave; e < end; e += kIaThreads / 64) {
        const int c = col[e];
        if ((unsigned)c >= (unsigned)n_cols) continue;                 // the wave's own entry: uniform
        double s = 0.0;
        for (int k = lane; k < d; k += 64) s += (double)x[k] * (double)Y[(size_t)c * d + k];
        s = wave_sum(s);
        if (lane == 0) {
#pragma clang fp contract(off)
            const float w = alpha * (float)(int)val[e];
            const float cc = 1.0f + w;
            acc += (double)cc * ((1.0 - s) * (1.0 - s)) - s * s;
        }
    }
    acc = block_sum_256(acc, red);
    if (tid == 0) partial[u] = acc;
}

// J = the rows' doubles (thread t sums rows t, t + 256, ... in order; the threads by block_sum_256) + lambda trace(GY)
__global__ __launch_bounds__(kIaThreads) void ials_objective_sum_kernel(int n_rows, int d, float lambda, const double *__restrict__ partial,
                                                                        const double *__restrict__ GY, double *__restrict__ J)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int u = threadIdx.x; u < n_rows; u += kIaThreads) acc += partial[u];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        double tr = 0.0;
        for (int k = 0; k < d; ++k) tr += GY[k * d + k];
        J[0] = acc + (double)lambda * tr;
    }
}

// ---- entries
// The row kernels take up to 66 KiB of LDS (d = 128): above the 64 KiB a kernel gets unasked.
static hipError_t ia_allow_lds()
{
    static RkPerDeviceOnce once;
    int dev;
    if (!once.need(&dev)) return hipSuccess;
#define IA_ATTR(NT)                                                                                                                   \
    do {                                                                                                                              \
        hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(ials_half_sweep_kernel<NT>),                               \
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMaxBytes - 64);                           \
        if (e_ == hipSuccess)                                                                                                         \
            e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(ials_system_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                     kLdsMaxBytes - 64);                                                                              \
        if (e_ != hipSuccess) return e_;                                                                                              \
    } while (0)
    IA_ATTR(1); IA_ATTR(2); IA_ATTR(3); IA_ATTR(4); IA_ATTR(5); IA_ATTR(6); IA_ATTR(7); IA_ATTR(8);
#undef IA_ATTR
    once.done(dev);
    return hipSuccess;
}

RK_EXPORT int rk_ials_gram(int32_t n, int32_t d, const float *Y, float lambda, float *G, float *work, int64_t work_floats, void *stream)
{
    if (n < 1 || !Y || !G || !work) RK_FAIL(RK_EINVAL, "rk_ials_gram: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_gram: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_lambda(lambda)) RK_FAIL(RK_EINVAL, "rk_ials_gram: lambda = %g is not a finite positive number", (double)lambda);
    const int dp = ia_dp(d), n_blocks = (n + kIaGramRows - 1) / kIaGramRows;
    if (work_floats < (int64_t)n_blocks * dp * dp)
        RK_FAIL(RK_EINVAL, "rk_ials_gram: a workspace of %lld floats, %lld needed (%d blocks x %d x %d)", (long long)work_floats,
                (long long)n_blocks * dp * dp, n_blocks, dp, dp);
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = sizeof(float) * ia_lds_floats(dp, false);
#define IA_CALL(NT) hipLaunchKernelGGL(ials_gram_partial_kernel<NT>, dim3(n_blocks), dim3(kIaThreads), lds, s, n, d, Y, work)
    IA_DISPATCH(dp / 16, IA_CALL);
#undef IA_CALL
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(ials_gram_finish_kernel, dim3((d * d + kIaThreads - 1) / kIaThreads), dim3(kIaThreads), 0, s, n_blocks, d, dp, work,
                       lambda, G);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_ials_gram64(int32_t n, int32_t d, const float *Y, double *GY, void *stream)
{
    if (n < 1 || !Y || !GY) RK_FAIL(RK_EINVAL, "rk_ials_gram64: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_gram64: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    hipStream_t s = (hipStream_t)stream;
    const int rows = ia_gram64_rows(n), n_blocks = (n + rows - 1) / rows;
    RkScratch scratch(s);
    double *part;
    RK_HIP(scratch.get(&part, (size_t)n_blocks * d * d));
    hipLaunchKernelGGL(ials_gram64_partial_kernel, dim3(n_blocks), dim3(kIaThreads), 0, s, n, d, rows, Y, part);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(ials_gram64_finish_kernel, dim3((d * d + kIaThreads - 1) / kIaThreads), dim3(kIaThreads), 0, s, n_blocks, d, part, GY);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_ials_system(int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col, const float *val,
                             float alpha, const float *Y, int32_t nb, const int32_t *row_ids, float *A_out, float *b_out, void *stream)
{
    if (n_cols < 1 || nb < 0 || !G || !rowptr || !col || !val || !Y) RK_FAIL(RK_EINVAL, "rk_ials_system: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_system: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(alpha)) RK_FAIL(RK_EINVAL, "rk_ials_system: alpha = %g is not a finite number >= 0", (double)alpha);
    if (nb == 0) return RK_OK;
    if (!row_ids || !A_out || !b_out) RK_FAIL(RK_EINVAL, "rk_ials_system: bad arguments");
    RK_HIP(ia_allow_lds());
    const int dp = ia_dp(d);
    const size_t lds = sizeof(float) * ia_lds_floats(dp, true);
#define IA_CALL(NT)                                                                                                                     \
    hipLaunchKernelGGL(ials_system_kernel<NT>, dim3(nb), dim3(kIaThreads), lds, (hipStream_t)stream, n_cols, d, G, rowptr, col, val, alpha, Y, \
                       row_ids, A_out, b_out)
    IA_DISPATCH(dp / 16, IA_CALL);
#undef IA_CALL
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_ials_half_sweep(int32_t n_rows, int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col,
                                 const float *val, float alpha, const float *Y, const int32_t *order, float *X_out, int32_t *status,
                                 void *stream)
{
    if (n_rows < 1 || n_cols < 1 || !G || !rowptr || !col || !val || !Y || !X_out || !status)
        RK_FAIL(RK_EINVAL, "rk_ials_half_sweep: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_half_sweep: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(alpha)) RK_FAIL(RK_EINVAL, "rk_ials_half_sweep: alpha = %g is not a finite number >= 0", (double)alpha);
    RK_HIP(ia_allow_lds());
    hipStream_t s = (hipStream_t)stream;
    const int dp = ia_dp(d);
    const size_t lds = sizeof(float) * ia_lds_floats(dp, true);
    RK_HIP(rk_set_status(status, 0, -1, s));
#define IA_CALL(NT)                                                                                                                   \
    hipLaunchKernelGGL(ials_half_sweep_kernel<NT>, dim3(n_rows), dim3(kIaThreads), lds, s, n_rows, n_cols, d, G, rowptr, col, val, alpha, Y, \
                       order, X_out, status)
    IA_DISPATCH(dp / 16, IA_CALL);
#undef IA_CALL
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_ials_objective(int32_t n_rows, int32_t n_cols, int32_t d, const int32_t *rowptr, const int32_t *col, const float *val,
                                float alpha, float lambda, const float *X, const float *Y, const double *GY, double *partial, double *J,
                                void *stream)
{
    if (n_rows < 1 || n_cols < 1 || !rowptr || !col || !val || !X || !Y || !GY || !partial || !J)
        RK_FAIL(RK_EINVAL, "rk_ials_objective: bad arguments");
    if (ia_bad_dim(d)) RK_FAIL(RK_EINVAL, "rk_ials_objective: d = %d outside 1..%d", d, RK_IALS_MAX_DIM);
    if (ia_bad_alpha(alpha)) RK_FAIL(RK_EINVAL, "rk_ials_objective: alpha = %g is not a finite number >= 0", (double)alpha);
    if (ia_bad_lambda(lambda)) RK_FAIL(RK_EINVAL, "rk_ials_objective: lambda = %g is not a finite positive number", (double)lambda);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ials_objective_kernel, dim3(n_rows), dim3(kIaThreads), 0, s, n_cols, d, rowptr, col, val, alpha, lambda, X, Y, GY, partial);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(ials_objective_sum_kernel, dim3(1), dim3(kIaThreads), 0, s, n_rows, d, lambda, partial, GY, J);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
