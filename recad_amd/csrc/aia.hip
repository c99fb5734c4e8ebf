// AIA attacker (recad/model/attacker/aia.py) on the device: the weighted-MF surrogate it trains from scratch on every
// train_step, the reverse pass through its last (unrolled) Adam epochs, the attack loss and the generator's Adam step.
//
// Nothing U x I, B x I or R x I is formed.  The surrogate's data is one CSR of R = real users + fake rows: the rating CSR,
// then filler_num slots per fake row whose values are the projected generator (rk_aia_project).  weight_neg_s is 0, so
// only an entry with X > 0 enters the loss (weight_pos_s), and a WMF step only needs the batch's nonzeros.
//
// One forward step is ONE launch (wmf_step_kernel<FWD>): the first nb workgroups own the batch's P rows (one row per
// workgroup: residuals over the row, a fixed-order reduction of the row's gradient, its Adam update); the others walk all
// rows of [P; Q] in tiles of 256 / DP rows, give untouched rows their weight-decay-only Adam update and recompute, for an
// item row, the residuals of the batch rows that rated it (each lane of the item's group binary-searches one batch row,
// the group then adds them in batch order).  The state is read from one slot and written to the next, so no workgroup
// reads a row another one is updating; the unrolled epochs keep every slot (or checkpoints, see attack/aia.py).
// The reverse of one step is two launches: <REV_A> the element-wise adjoint of Adam (ḡ, m̄, v̄), then <REV_B> the batch
// part of θ̄ and of X̄ (the fake entries), with the same ownership.  No float atomics anywhere: every reduction has a
// fixed order, so two runs are bit-identical.
//
// Rows are padded to DP in {16, 32, 64} floats; the pad columns stay exactly 0 (zero init, zero gradient, Adam of 0 is 0).
#include <algorithm>

#include "common.h"

namespace {

enum { FWD = 0, REV_A = 1, REV_B = 2 };

struct StepArgs {
    int R, I, s0, nb;
    long long nnz_real;
    const int *rowptr, *col, *perm, *invperm;
    const float *x;
    const float *th, *m_in, *v_in;     // slot k: theta, m, v
    float *th_out, *m_out, *v_out;     // FWD: slot k + 1
    const float *mo, *vo;              // REV: m', v' of slot k + 1
    float *adj_th, *adj_m, *adj_v, *gbar, *xbar;
    float step_size, bc2s, b1, b2, eps, wd, w;
};

// sum over the DP lanes of a group; the xor butterfly leaves the same bits in every lane
template <int DP>
__device__ __forceinline__ float gsum(float v)
{
#pragma unroll
    for (int o = DP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, DP);
    return v;
}

__device__ __forceinline__ float wt(float x, float w) { return x > 0.f ? w : 0.f; }

// element (row, lane) once its batch part is known
template <int MODE>
__device__ __forceinline__ void elem_update(const StepArgs &a, long long idx, float bp)
{
    const float th = a.th[idx];
    if (MODE == FWD) {
        const float g = bp + a.wd * th;     // torch Adam: grad.add(param, alpha=weight_decay)
        float p = th, m = a.m_in[idx], v = a.v_in[idx];
        adam_elem(p, m, v, g, 1.f - a.b1, a.b2, 1.f - a.b2, a.step_size, a.bc2s, a.eps);
        a.th_out[idx] = p;
        a.m_out[idx] = m;
        a.v_out[idx] = v;
    } else if (MODE == REV_A) {
        // adjoint of  m' = b1 m + (1-b1) g,  v' = b2 v + (1-b2) g^2,  th' = th - alpha m' / (sqrt(v') / c2 + eps)
        const float g = bp + a.wd * th;
        const float mo = a.mo[idx], vo = a.vo[idx];
        const float thb = a.adj_th[idx], mb = a.adj_m[idx], vb = a.adj_v[idx];
        const float sv = sqrtf(vo);
        const float D = sv / a.bc2s + a.eps;
        const float mh = mb - a.step_size * thb / D;
        // d th' / d v' has a 1 / sqrt(v') factor; at v' == 0 (an entry whose gradient was exactly 0 on every step so far)
        // the term is taken as 0 -- autograd gives NaN there, and with weight decay > 0 it needs an exact-0 entry
        const float vh = vb + (vo > 0.f ? a.step_size * thb * mo / (2.f * a.bc2s * D * D * sv) : 0.f);
        const float gb = (1.f - a.b1) * mh + 2.f * (1.f - a.b2) * g * vh;
        a.adj_m[idx] = a.b1 * mh;
        a.adj_v[idx] = a.b2 * vh;
        a.gbar[idx] = gb;
    } else {
        a.adj_th[idx] = a.adj_th[idx] + a.wd * a.gbar[idx] + bp;
    }
}

template <int DP, int MODE>
__global__ __launch_bounds__(256) void wmf_step_kernel(StepArgs a)
{
    constexpr int G = 256 / DP;
    const int tid = threadIdx.x, gi = tid / DP, lane = tid % DP;
    const float w = a.w;
    if ((int)blockIdx.x < a.nb) {
        // ---- one batch row r: its residuals over the whole row
        __shared__ float red[256];
        const int r = a.perm[a.s0 + blockIdx.x];
        const long long pr = (long long)r * DP + lane;
        const float p = a.th[pr];
        const float gp = (MODE == REV_B) ? a.gbar[pr] : 0.f;
        float acc = 0.f;
        for (int k = a.rowptr[r] + gi; k < a.rowptr[r + 1]; k += G) {
            const float xk = a.x[k];
            const long long qi = (long long)(a.R + a.col[k]) * DP + lane;
            const float q = a.th[qi];
            const float e = xk - gsum<DP>(p * q);
            const float ww = wt(xk, w);
            if (MODE == REV_B) {
                const float gq = a.gbar[qi];
                const float av = gsum<DP>(gp * q + gq * p);
                acc += ww * (av * q - e * gq);
                if (lane == 0 && k >= a.nnz_real) a.xbar[k - a.nnz_real] += -2.f * ww * av;
            } else {
                acc += ww * e * q;
            }
        }
        red[tid] = acc;
        __syncthreads();
        if (gi == 0) {
            float s = 0.f;
            for (int q = 0; q < G; ++q) s += red[q * DP + lane];
            elem_update<MODE>(a, pr, MODE == REV_B ? 2.f * s : -2.f * s);
        }
        return;
    }
    // ---- a tile of rows of [P; Q]
    const int row = (blockIdx.x - a.nb) * G + gi;
    if (row >= a.R + a.I) return;
    const long long idx = (long long)row * DP + lane;
    if (row < a.R) {
        const int pos = a.invperm[row];
        if (pos >= a.s0 && pos < a.s0 + a.nb) return;     // a batch row: its own workgroup has it
        elem_update<MODE>(a, idx, 0.f);
        return;
    }
    const int item = row - a.R;
    const float q = a.th[idx];
    const float gq = (MODE == REV_B) ? a.gbar[idx] : 0.f;
    float acc = 0.f;
    for (int c0 = 0; c0 < a.nb; c0 += DP) {
        int kpos = -1;
        if (c0 + lane < a.nb) {
            const int rj = a.perm[a.s0 + c0 + lane];
            kpos = rk_find_sorted(a.col, a.rowptr[rj], a.rowptr[rj + 1], item);
        }
        const int n = min(DP, a.nb - c0);
        for (int jj = 0; jj < n; ++jj) {
            const int k = __shfl(kpos, jj, DP);
            if (k < 0) continue;
            const int rj = a.perm[a.s0 + c0 + jj];
            const long long pj = (long long)rj * DP + lane;
            const float p = a.th[pj];
            const float xk = a.x[k];
            const float e = xk - gsum<DP>(p * q);
            const float ww = wt(xk, w);
            if (MODE == REV_B) {
                const float gp = a.gbar[pj];
                const float av = gsum<DP>(gp * q + gq * p);
                acc += ww * (av * p - e * gp);
            } else {
                acc += ww * e * p;
            }
        }
    }
    elem_update<MODE>(a, idx, MODE == REV_B ? 2.f * acc : -2.f * acc);
}

// ---------------------------------------------------------------- attack loss (aia.py:13-20, 88-114)
// s_ui = p_u . q_i as one explicit fma chain, so every kernel below gets the same bits for the same (u, i)
template <int DP>
__device__ __forceinline__ float dotp(const float *p, const float *__restrict__ q)
{
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DP; ++d) s = __builtin_fmaf(p[d], q[d], s);
    return s;
}

// one wave per (target, user) pair: the masked log-sum-exp of z_ui = s_ui [s_ui >= s_ut], and the pair's loss
template <int DP>
__global__ __launch_bounds__(256) void loss_lse_kernel(int n_pairs, int R, int I, const int *__restrict__ pair_user,
                                                       const int *__restrict__ pair_tgt, const float *__restrict__ th,
                                                       float *__restrict__ lse, float *__restrict__ sut, float *__restrict__ ploss)
{
    const int pi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pi >= n_pairs) return;
    float p[DP];
    const float *pu = th + (long long)pair_user[pi] * DP;
#pragma unroll
    for (int d = 0; d < DP; ++d) p[d] = pu[d];
    const int t = pair_tgt[pi];
    const float *Q = th + (long long)R * DP;
    const float st = dotp<DP>(p, Q + (long long)t * DP);
    float mx = -INFINITY, sm = 0.f;
    for (int i = lane; i < I; i += 64) {
        const float s = dotp<DP>(p, Q + (long long)i * DP);
        const float z = (i == t || s >= st) ? s : 0.f;
        if (z > mx) {
            sm = sm * expf(mx - z) + 1.f;
            mx = z;
        } else {
            sm += expf(z - mx);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float mo = __shfl_xor(mx, o, 64), so = __shfl_xor(sm, o, 64);
        const float m2 = fmaxf(mx, mo);
        sm = (mx == -INFINITY ? 0.f : sm * expf(mx - m2)) + (mo == -INFINITY ? 0.f : so * expf(mo - m2));
        mx = m2;
    }
    if (lane == 0) {
        const float l = mx + logf(sm);
        lse[pi] = l;
        sut[pi] = st;
        ploss[pi] = -(st - l) / 1.1f;
    }
}

// dF/ds_ui = (M_ui softmax(z_u)_i - [i = t]) / (11 |T_t|)
__device__ __forceinline__ float dfds(float s, int i, int t, float st, float l, float sc)
{
    const bool M = (i == t) || s >= st;
    return ((M ? expf(s - l) : 0.f) - (i == t ? 1.f : 0.f)) * sc;
}

// one wave per real user u: p̄_u = sum over its pairs, over i, of dF/ds_ui q_i
template <int DP>
__global__ __launch_bounds__(256) void loss_pgrad_kernel(int U, int R, int I, int n_tgt, const int *__restrict__ tgt,
                                                         const int *__restrict__ pidx, const float *__restrict__ tscale,
                                                         const float *__restrict__ th, const float *__restrict__ lse,
                                                         const float *__restrict__ sut, float *__restrict__ adj)
{
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= U) return;
    float p[DP], acc[DP];
    const float *pu = th + (long long)u * DP;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        p[d] = pu[d];
        acc[d] = 0.f;
    }
    const float *Q = th + (long long)R * DP;
    for (int tt = 0; tt < n_tgt; ++tt) {
        const int pi = pidx[(long long)tt * U + u];
        if (pi < 0) continue;
        const int t = tgt[tt];
        const float st = sut[pi], l = lse[pi], sc = tscale[tt];
        for (int i = lane; i < I; i += 64) {
            const float *qi = Q + (long long)i * DP;
            const float gs = dfds(dotp<DP>(p, qi), i, t, st, l, sc);
#pragma unroll
            for (int d = 0; d < DP; ++d) acc[d] += gs * qi[d];
        }
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const float v = wave_sum(acc[d]);
        if (lane == 0) adj[(long long)u * DP + d] = v;
    }
}

// one wave per item i: q̄_i = sum over all pairs (u, t), in pair order, of dF/ds_ui p_u
template <int DP>
__global__ __launch_bounds__(256) void loss_qgrad_kernel(int n_pairs, int R, int I, const int *__restrict__ pair_user,
                                                         const int *__restrict__ pair_tgt, const int *__restrict__ pair_slot,
                                                         const float *__restrict__ tscale, const float *__restrict__ th,
                                                         const float *__restrict__ lse, const float *__restrict__ sut,
                                                         float *__restrict__ adj)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= I) return;
    const float *qi = th + (long long)(R + i) * DP;
    float acc[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) acc[d] = 0.f;
    for (int pi = lane; pi < n_pairs; pi += 64) {
        const float *pu = th + (long long)pair_user[pi] * DP;
        float p[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) p[d] = pu[d];
        const float gs = dfds(dotp<DP>(p, qi), i, pair_tgt[pi], sut[pi], lse[pi], tscale[pair_slot[pi]]);
#pragma unroll
        for (int d = 0; d < DP; ++d) acc[d] += gs * p[d];
    }
#pragma unroll
    for (int d = 0; d < DP; ++d) {
        const float v = wave_sum(acc[d]);
        if (lane == 0) adj[(long long)(R + i) * DP + d] = v;
    }
}

// G_loss = sum_t mean_u(pair loss) / 10, as one device scalar
__global__ void loss_sum_kernel(int n_tgt, const int *__restrict__ pair_ptr, const float *__restrict__ ploss, float *__restrict__ out)
{
    const int lane = threadIdx.x;
    float total = 0.f;
    for (int tt = 0; tt < n_tgt; ++tt) {
        const int b = pair_ptr[tt], e = pair_ptr[tt + 1];
        float s = 0.f;
        for (int k = b + lane; k < e; k += 64) s += ploss[k];
        s = wave_sum(s);
        total += s / (float)(e - b);
    }
    if (lane == 0) out[0] = total / 10.f;
}

// project (aia.py:534-549): round half to even, then clamp to [0, 5]
__global__ void project_kernel(int n, const float *__restrict__ gen, float *__restrict__ x)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float v = rintf(gen[k]);
    v = v < 0.f ? 0.f : v;
    v = v > 5.f ? 5.f : v;
    x[k] = v;
}

__global__ void g_adam_kernel(int n, float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                              const float *__restrict__ grad, float step_size, float bc2s, float b1, float b2, float eps)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float pp = p[k], mm = m[k], vv = v[k];
    adam_elem(pp, mm, vv, grad[k], 1.f - b1, b2, 1.f - b2, step_size, bc2s, eps);
    p[k] = pp;
    m[k] = mm;
    v[k] = vv;
}

int check_desc(const rk_aia_desc *d, const char *who)
{
    if (!d || d->n_rows <= 0 || d->n_real <= 0 || d->n_real > d->n_rows || d->n_items <= 0 || d->batch <= 0 ||
        d->batch > RK_AIA_MAX_BATCH || !(d->dpad == 16 || d->dpad == 32 || d->dpad == 64) || d->nnz_real < 0 || !d->rowptr ||
        !d->col || !d->x)
        RK_FAIL(RK_EINVAL, "%s: bad descriptor", who);
    return RK_OK;
}

long long state_floats(const rk_aia_desc *d) { return (long long)(d->n_rows + d->n_items) * d->dpad; }

StepArgs step_args(const rk_aia_desc *d, const int32_t *perm, const int32_t *invperm, int j, int adam_t)
{
    StepArgs a{};
    a.R = d->n_rows;
    a.I = d->n_items;
    a.s0 = j * d->batch;
    a.nb = std::min(d->batch, d->n_rows - a.s0);
    a.nnz_real = d->nnz_real;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.perm = perm;
    a.invperm = invperm;
    a.x = d->x;
    const AdamCoef c = adam_coef(adam_t, d->lr, d->beta1, d->beta2);
    a.step_size = c.step_size;
    a.bc2s = c.bc2s;
    a.b1 = d->beta1;
    a.b2 = d->beta2;
    a.eps = d->eps;
    a.wd = d->wd;
    a.w = d->w_pos;
    return a;
}

template <int MODE>
int launch_step(const rk_aia_desc *d, const StepArgs &a, hipStream_t s)
{
    const int G = 256 / d->dpad;
    const int grid = a.nb + (a.R + a.I + G - 1) / G;
    switch (d->dpad) {
    case 16: hipLaunchKernelGGL((wmf_step_kernel<16, MODE>), dim3(grid), dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((wmf_step_kernel<32, MODE>), dim3(grid), dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((wmf_step_kernel<64, MODE>), dim3(grid), dim3(256), 0, s, a); break;
    }
    RK_CHECK_LAUNCH();
    return RK_OK;
}

int check_range(const rk_aia_desc *d, int32_t lo, int32_t hi, int32_t adam_t_lo, const char *who)
{
    const int nsteps = (d->n_rows + d->batch - 1) / d->batch;
    if (lo < 0 || hi > nsteps || lo > hi || adam_t_lo < 1)
        RK_FAIL(RK_EINVAL, "%s: bad step range [%d, %d) of %d (adam_t %d)", who, lo, hi, nsteps, adam_t_lo);
    return RK_OK;
}

}  // namespace

RK_EXPORT int rk_aia_project(int32_t n, const float *gen, float *x, void *stream)
{
    if (n < 0 || (n > 0 && (!gen || !x))) RK_FAIL(RK_EINVAL, "rk_aia_project: bad arguments");
    if (n == 0) return RK_OK;
    hipLaunchKernelGGL(project_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, gen, x);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aia_forward(const rk_aia_desc *d, const int32_t *perm, const int32_t *invperm, int32_t lo, int32_t hi, int32_t adam_t_lo,
                             float *slots, int32_t keep_all, int32_t parity0, void *stream)
{
    if (int rc = check_desc(d, "rk_aia_forward")) return rc;
    if (int rc = check_range(d, lo, hi, adam_t_lo, "rk_aia_forward")) return rc;
    if (!perm || !invperm || !slots || parity0 < 0 || parity0 > 1) RK_FAIL(RK_EINVAL, "rk_aia_forward: bad arguments");
    const long long N = state_floats(d), stride = 3 * N;
    hipStream_t s = (hipStream_t)stream;
    for (int j = lo; j < hi; ++j) {
        StepArgs a = step_args(d, perm, invperm, j, adam_t_lo + (j - lo));
        const long long in = keep_all ? (long long)(j - lo) : (long long)((parity0 + j - lo) & 1);
        const long long out = keep_all ? in + 1 : 1 - in;
        float *si = slots + in * stride, *so = slots + out * stride;
        a.th = si;
        a.m_in = si + N;
        a.v_in = si + 2 * N;
        a.th_out = so;
        a.m_out = so + N;
        a.v_out = so + 2 * N;
        if (int rc = launch_step<FWD>(d, a, s)) return rc;
    }
    return RK_OK;
}

RK_EXPORT int rk_aia_reverse(const rk_aia_desc *d, const int32_t *perm, const int32_t *invperm, int32_t lo, int32_t hi, int32_t adam_t_lo,
                             const float *slots, float *adj, float *gbar, float *xbar, void *stream)
{
    if (int rc = check_desc(d, "rk_aia_reverse")) return rc;
    if (int rc = check_range(d, lo, hi, adam_t_lo, "rk_aia_reverse")) return rc;
    if (!perm || !invperm || !slots || !adj || !gbar || (d->n_rows > d->n_real && d->n_fake_nz > 0 && !xbar))
        RK_FAIL(RK_EINVAL, "rk_aia_reverse: bad arguments");
    const long long N = state_floats(d), stride = 3 * N;
    hipStream_t s = (hipStream_t)stream;
    for (int j = hi - 1; j >= lo; --j) {
        StepArgs a = step_args(d, perm, invperm, j, adam_t_lo + (j - lo));
        const float *si = slots + (long long)(j - lo) * stride, *so = si + stride;
        a.th = si;
        a.mo = so + N;
        a.vo = so + 2 * N;
        a.adj_th = adj;
        a.adj_m = adj + N;
        a.adj_v = adj + 2 * N;
        a.gbar = gbar;
        a.xbar = xbar;
        if (int rc = launch_step<REV_A>(d, a, s)) return rc;
        if (int rc = launch_step<REV_B>(d, a, s)) return rc;
    }
    return RK_OK;
}

RK_EXPORT int rk_aia_attack_loss(const rk_aia_desc *d, int32_t n_tgt, const int32_t *tgt, const int32_t *pair_ptr, int32_t n_pairs,
                                 const int32_t *pair_user, const int32_t *pair_tgt, const int32_t *pair_slot, const int32_t *pidx,
                                 const float *tscale, const float *theta, float *work, float *loss, float *adj, void *stream)
{
    if (int rc = check_desc(d, "rk_aia_attack_loss")) return rc;
    if (n_tgt <= 0 || n_pairs <= 0 || !tgt || !pair_ptr || !pair_user || !pair_tgt || !pair_slot || !pidx || !tscale || !theta || !work ||
        !loss || !adj)
        RK_FAIL(RK_EINVAL, "rk_aia_attack_loss: bad arguments (%d targets, %d pairs)", n_tgt, n_pairs);
    hipStream_t s = (hipStream_t)stream;
    const long long N = state_floats(d);
    RK_HIP(rk_zero_async(adj, sizeof(float) * (size_t)(3 * N), s));
    float *lse = work, *sut = work + n_pairs, *pl = work + 2LL * n_pairs;
    const int R = d->n_rows, I = d->n_items, U = d->n_real;
#define RK_AIA_LOSS(DP)                                                                                                             \
    hipLaunchKernelGGL(loss_lse_kernel<DP>, dim3((n_pairs + 3) / 4), dim3(256), 0, s, n_pairs, R, I, pair_user, pair_tgt, theta, lse, \
                       sut, pl);                                                                                                    \
    RK_CHECK_LAUNCH();                                                                                                              \
    hipLaunchKernelGGL(loss_pgrad_kernel<DP>, dim3((U + 3) / 4), dim3(256), 0, s, U, R, I, n_tgt, tgt, pidx, tscale, theta, lse, sut, adj); \
    RK_CHECK_LAUNCH();                                                                                                              \
    hipLaunchKernelGGL(loss_qgrad_kernel<DP>, dim3((I + 3) / 4), dim3(256), 0, s, n_pairs, R, I, pair_user, pair_tgt, pair_slot, tscale,   \
                       theta, lse, sut, adj);                                                                                       \
    RK_CHECK_LAUNCH();
    switch (d->dpad) {
    case 16: RK_AIA_LOSS(16) break;
    case 32: RK_AIA_LOSS(32) break;
    default: RK_AIA_LOSS(64) break;
    }
#undef RK_AIA_LOSS
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(64), 0, s, n_tgt, pair_ptr, pl, loss);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aia_g_step(int32_t n, float *gen, float *m, float *v, const float *grad, int32_t adam_t, float lr, float beta1, float beta2,
                            float eps, void *stream)
{
    if (n < 0 || adam_t < 1 || (n > 0 && (!gen || !m || !v || !grad))) RK_FAIL(RK_EINVAL, "rk_aia_g_step: bad arguments");
    if (n == 0) return RK_OK;
    const AdamCoef c = adam_coef(adam_t, lr, beta1, beta2);
    hipLaunchKernelGGL(g_adam_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, gen, m, v, grad, c.step_size, c.bc2s,
                       beta1, beta2, eps);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
