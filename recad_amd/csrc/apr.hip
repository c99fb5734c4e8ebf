// APR victim: BPR matrix factorisation with an adversarial second term (He et al., SIGIR 2018); include/recad_hip.h states the
// definition.  A step needs two row-grouped sums (Gamma, then the gradient of L + adv_reg L' + R), each complete per row
// before it is used and each in a fixed order, so that a training run is repeatable to the bit.  Nothing here adds floats
// atomically: the epoch's incidences (step, row, 3 b + role) are sorted once, a pass over the sorted keys gives every touched
// row of a step a compact slot, and one wave per slot walks the row's run in key order, re-reading the partner rows (no
// contribution rows are stored: a contribution is c_b times a row that is in the table anyway).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "common.h"

// steps 2 and 5 round every product and every addition on its own; the norms may not be contracted differently from one
// kernel to the next either, so the whole file is compiled without contraction
#pragma clang fp contract(off)

static constexpr int kAprIncBits = 20, kAprRowBits = 24, kAprStepBits = 20;   // the key of lightgcn.hip's plan
static constexpr int kAprGroup = 16;                                           // lanes per triplet in the coefficient kernels
static constexpr int kAprTripletsPerBlock = 256 / kAprGroup;
static_assert(RK_APR_MAX_DIM == 4 * kWave, "a lane of the row kernels holds 1, 2 or 4 elements of a row");
static_assert(3LL * RK_APR_MAX_BATCH < (1LL << kAprIncBits), "3 b + role must fit the key's low bits");

__device__ __forceinline__ int apr_key_row(unsigned long long k) { return (int)((k >> kAprIncBits) & ((1ULL << kAprRowBits) - 1)); }
__device__ __forceinline__ int apr_key_inc(unsigned long long k) { return (int)(k & ((1ULL << kAprIncBits) - 1)); }

// ---- validation: reads the id arrays only.  First offending (triplet, rule) by rk_record_bad.
__global__ void apr_check_kernel(const int64_t *__restrict__ users, const int64_t *__restrict__ pos, const int64_t *__restrict__ neg,
                                 long long n, int U, int I, unsigned long long *__restrict__ first_bad)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int64_t u = users[t], i = pos[t], j = neg[t];
        int rule = 0;
        if (u < 0 || u >= U) rule = RK_APR_BAD_USER;
        else if (i < 0 || i >= I) rule = RK_APR_BAD_POS;
        else if (j < 0 || j >= I) rule = RK_APR_BAD_NEG;
        if (rule) rk_record_bad(first_bad, t, rule);
    }
}

// ---- the plan
__global__ void apr_keys_kernel(const int64_t *__restrict__ users, const int64_t *__restrict__ pos, const int64_t *__restrict__ neg,
                                long long n, int batch, int U, unsigned long long *__restrict__ keys)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const unsigned long long step = (unsigned long long)(t / batch), b3 = 3ULL * (unsigned long long)(t % batch);
        const unsigned long long hi = step << (kAprIncBits + kAprRowBits);
        keys[3 * t + 0] = hi | ((unsigned long long)users[t] << kAprIncBits) | (b3 + 0);
        keys[3 * t + 1] = hi | ((unsigned long long)(U + pos[t]) << kAprIncBits) | (b3 + 1);
        keys[3 * t + 2] = hi | ((unsigned long long)(U + neg[t]) << kAprIncBits) | (b3 + 2);
    }
}

// One workgroup per step: the sorted positions at which a row's run starts, compacted in order.  run[0] = n_runs,
// run[1 + k] = start of slot k, run[1 + n_runs] = 3 nb.
__global__ __launch_bounds__(256) void apr_runs_kernel(const unsigned long long *__restrict__ keys, long long n, int batch, int run_stride,
                                                       int *__restrict__ run_all)
{
    __shared__ int wave_cnt[4];
    const long long step = blockIdx.x;
    const long long first = step * batch;
    const int cnt = 3 * (int)(n - first < batch ? n - first : batch);
    const unsigned long long *k = keys + 3 * first;
    int *run = run_all + step * run_stride;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int done = 0;
    for (int base = 0; base < cnt; base += 256) {
        const int p = base + (int)threadIdx.x;
        const bool head = p < cnt && (p == 0 || apr_key_row(k[p]) != apr_key_row(k[p - 1]));
        const unsigned long long mask = __ballot(head);
        if (lane == 0) wave_cnt[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { if (q < w) before += wave_cnt[q]; total += wave_cnt[q]; }
        if (head) run[1 + done + before + __popcll(mask & ((1ULL << lane) - 1ULL))] = p;
        done += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { run[0] = done; run[1 + done] = cnt; }
}

// ---- per step
struct AprStep {
    const float *table;
    const int64_t *users, *pos, *neg;     // the step's triplets
    const unsigned long long *keys;       // the step's sorted incidences
    const int *run;                       // the step's run table
    int nb, U, d;
    float eps, adv_reg, lam_b;            // lam_b = fl(lambda / (float) nb)
    float *x, *c, *x_adv, *c_adv, *gamma, *norm, *delta, *grad;
    int *slot_of;
    double *part;
    int part_blocks;
};

// sum over the 16 lanes of a triplet's group; every lane of the group gets it
__device__ __forceinline__ double apr_group_sum(double v)
{
#pragma unroll
    for (int o = kAprGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x, c and the partial sums of L (and of R when ADV == 0) per triplet: 16 lanes each.  VEC4: dim == 64, one float4 per lane.
// ADV: the rows are moved by their Delta first (step 4), each element fl(q + Delta) as the gradient kernel forms it.
// The dots, sigma and softplus are worked out in double and rounded once: the products of two floats are exact there, so x and c
// are the correctly rounded values of the fp32 rows but for the last bits of a 16-lane tree of doubles.  This costs a few fp64
// operations per lane, and it matters: Adam divides by sqrt(v), and over the first steps of a training a last-bit error of c
// is what moves the tables furthest from the float64 run.
// The bodies take the step record and the workgroup's index in the step's own grid: rk_apr_train_epoch launches them one model at
// a time, rk_apr_train_epoch_group with the member as the grid's second dimension.
template <bool VEC4, bool ADV>
__device__ __forceinline__ void apr_coef_body(const AprStep &a, const int block, double *red)
{
    const int g = threadIdx.x / kAprGroup, l = threadIdx.x % kAprGroup;
    const int b = block * kAprTripletsPerBlock + g;
    double sp = 0.0, sq = 0.0;
    if (b < a.nb) {
        const int d = a.d;
        const float *pu = a.table + (size_t)a.users[b] * d;
        const float *qi = a.table + (size_t)(a.U + a.pos[b]) * d;
        const float *qj = a.table + (size_t)(a.U + a.neg[b]) * d;
        const float *du = nullptr, *di = nullptr, *dj = nullptr;
        if (ADV) {
            du = a.delta + (size_t)a.slot_of[3 * b + 0] * d;
            di = a.delta + (size_t)a.slot_of[3 * b + 1] * d;
            dj = a.delta + (size_t)a.slot_of[3 * b + 2] * d;
        }
        double dn = 0.0, dp = 0.0;
        auto add = [&](float p, float qa, float qb) {
            const double P = p, A = qa, Bq = qb;
            dn += P * Bq;
            dp += P * A;
            if (!ADV) sq += (P * P + A * A) + Bq * Bq;
        };
        if (VEC4) {
            float4 p = reinterpret_cast<const float4 *>(pu)[l], qa = reinterpret_cast<const float4 *>(qi)[l], qb = reinterpret_cast<const float4 *>(qj)[l];
            if (ADV) {
                const float4 e = reinterpret_cast<const float4 *>(du)[l], ea = reinterpret_cast<const float4 *>(di)[l], eb = reinterpret_cast<const float4 *>(dj)[l];
                p.x += e.x; p.y += e.y; p.z += e.z; p.w += e.w;
                qa.x += ea.x; qa.y += ea.y; qa.z += ea.z; qa.w += ea.w;
                qb.x += eb.x; qb.y += eb.y; qb.z += eb.z; qb.w += eb.w;
            }
            add(p.x, qa.x, qb.x); add(p.y, qa.y, qb.y); add(p.z, qa.z, qb.z); add(p.w, qa.w, qb.w);
        } else {
            for (int k = l; k < d; k += kAprGroup) {
                float p = pu[k], qa = qi[k], qb = qj[k];
                if (ADV) { p += du[k]; qa += di[k]; qb += dj[k]; }
                add(p, qa, qb);
            }
        }
        dn = apr_group_sum(dn);
        dp = apr_group_sum(dp);
        if (!ADV) sq = apr_group_sum(sq);
        const double x = dn - dp;
        if (l == 0) {
            (ADV ? a.x_adv : a.x)[b] = (float)x;
            (ADV ? a.c_adv : a.c)[b] = (float)(1.0 / (1.0 + exp(-x)) / (double)a.nb);
            sp = (x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x)));
        } else {
            sq = 0.0;
        }
    }
    const double s = block_sum_256(sp, red);
    if (ADV) {
        if (threadIdx.x == 0) a.part[2 * a.part_blocks + block] = s;
    } else {
        const double r = block_sum_256(sq, red);
        if (threadIdx.x == 0) { a.part[block] = s; a.part[a.part_blocks + block] = r; }
    }
}

template <bool VEC4, bool ADV>
__global__ __launch_bounds__(256) void apr_coef_kernel(AprStep a)
{
    __shared__ double red[4];
    apr_coef_body<VEC4, ADV>(a, blockIdx.x, red);
}

// One wave per touched row (slot).  The run is walked 64 incidences at a time: lane i loads incidence i's (b, role, c_b) and
// the rows of its partners, then the values are broadcast one incidence after the other and every lane accumulates its
// elements k = lane + 64 j of the row in key order.
// GRAD == 0: Gamma (step 2), its norm, Delta (step 3) and slot_of.  GRAD == 1: the row of step 5 into the dense gradient.
template <bool GRAD, int REGS>
__device__ __forceinline__ void apr_rows_body(const AprStep &a, const int block)
{
    const int lane = threadIdx.x & 63, slot = block * 4 + (threadIdx.x >> 6);
    if (slot >= a.run[0]) return;
    const int beg = a.run[1 + slot], end = a.run[2 + slot], d = a.d;
    const int row = apr_key_row(a.keys[beg]);
    const bool adv = GRAD && a.adv_reg != 0.f;
    float acc[REGS], self[REGS];
#pragma unroll
    for (int j = 0; j < REGS; ++j) {
        acc[j] = 0.f;
        const int k = lane + kWave * j;
        self[j] = (GRAD && k < d) ? a.table[(size_t)row * d + k] : 0.f;
    }
    for (int base = beg; base < end; base += kWave) {
        const int m = end - base < kWave ? end - base : kWave;
        int my_role = 0, my_r0 = 0, my_r1 = 0, my_s0 = 0, my_s1 = 0;
        float my_c = 0.f, my_ca = 0.f;
        if (lane < m) {
            const int inc = apr_key_inc(a.keys[base + lane]), b = inc / 3;
            my_role = inc - 3 * b;
            my_c = a.c[b];
            if (my_role == 0) { my_r0 = a.U + (int)a.pos[b]; my_r1 = a.U + (int)a.neg[b]; }
            else my_r0 = (int)a.users[b];
            if (!GRAD) a.slot_of[inc] = slot;
            if (adv) {
                my_ca = a.c_adv[b];
                if (my_role == 0) { my_s0 = a.slot_of[3 * b + 1]; my_s1 = a.slot_of[3 * b + 2]; }
                else my_s0 = a.slot_of[3 * b];
            }
        }
        for (int i = 0; i < m; ++i) {
            const int role = __shfl(my_role, i, 64), r0 = __shfl(my_r0, i, 64), r1 = __shfl(my_r1, i, 64);
            const float c = __shfl(my_c, i, 64);
            const float *t0 = a.table + (size_t)r0 * d, *t1 = a.table + (size_t)r1 * d;
            // the user's term is c (q_j - q_i): t0 = q_i, t1 = q_j; an item's is -c p_u (positive) or c p_u (negative): t0 = p_u
            const float cs = role == 1 ? -c : c;
            float ca = 0.f;
            const float *e0 = nullptr, *e1 = nullptr;
            if (adv) {
                const float v = __shfl(my_ca, i, 64);
                ca = role == 1 ? -v : v;
                e0 = a.delta + (size_t)__shfl(my_s0, i, 64) * d;
                e1 = a.delta + (size_t)__shfl(my_s1, i, 64) * d;
            }
#pragma unroll
            for (int j = 0; j < REGS; ++j) {
                const int k = lane + kWave * j;
                if (k < d) {
                    const float v0 = t0[k];
                    float v1 = 0.f;
                    if (role == 0) v1 = t1[k];
                    const float part = role == 0 ? v1 - v0 : v0;
                    acc[j] = acc[j] + cs * part;
                    if (GRAD) {
                        if (adv) {
                            const float w0 = v0 + e0[k];
                            float w1 = 0.f;
                            if (role == 0) w1 = v1 + e1[k];
                            const float part_a = role == 0 ? w1 - w0 : w0;
                            acc[j] = acc[j] + a.adv_reg * (ca * part_a);
                        }
                        acc[j] = acc[j] + a.lam_b * self[j];
                    }
                }
            }
        }
    }
    if (GRAD) {
#pragma unroll
        for (int j = 0; j < REGS; ++j) {
            const int k = lane + kWave * j;
            if (k < d) a.grad[(size_t)row * d + k] = acc[j];
        }
        return;
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < REGS; ++j) ss += acc[j] * acc[j];      // the elements past d are +0.0
    const float nr = sqrtf(wave_sum(ss));
    const float s = nr > 0.f ? a.eps / fmaxf(nr, 1e-12f) : 0.f;      // a zero row stays zero even where eps / 1e-12 overflows
    if (lane == 0) a.norm[slot] = nr;
#pragma unroll
    for (int j = 0; j < REGS; ++j) {
        const int k = lane + kWave * j;
        if (k < d) {
            a.gamma[(size_t)slot * d + k] = acc[j];
            a.delta[(size_t)slot * d + k] = acc[j] * s;
        }
    }
}

template <bool GRAD, int REGS>
__global__ __launch_bounds__(256) void apr_rows_kernel(AprStep a)
{
    apr_rows_body<GRAD, REGS>(a, blockIdx.x);
}

// The Adam pass over all N * d elements: reads g and stores 0 in its place, copies it out when asked, updates when asked.
// Workgroup 0 also adds the step's loss partials in a fixed order: losses = {L, L', R}.
// block of n_blocks: the workgroup's place in the pass over this model's elements
__device__ __forceinline__ void apr_adam_body(long long n, float *p, float *g, float *m, float *v, float *grad_out, int apply_update,
                                              float step_size, float bc2s, float b1, float b2, float eps, const double *part,
                                              int part_blocks, int used_blocks, int nb, float lam, int adv, double *losses, const int block,
                                              const int n_blocks, double *red)
{
    const float w1 = (float)(1.0 - (double)b1), w2 = (float)(1.0 - (double)b2);
    for (long long i = (long long)block * blockDim.x + threadIdx.x; i < n; i += (long long)n_blocks * blockDim.x) {
        const float gi = g[i];
        g[i] = 0.f;
        if (grad_out) grad_out[i] = gi;
        if (apply_update) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_elem(pp, mm, vv, gi, w1, b2, w2, step_size, bc2s, eps);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
    if (block != 0) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 3; ++q) {
        if (q == 2 && !adv) break;
        double t = 0.0;
        for (int i = threadIdx.x; i < used_blocks; i += 256) t += part[q * part_blocks + i];
        s[q] = block_sum_256(t, red);
    }
    if (threadIdx.x == 0) {
        losses[0] = s[0] / (double)nb;
        losses[1] = s[2] / (double)nb;
        losses[2] = (double)lam * 0.5 * s[1] / (double)nb;
    }
}

__global__ __launch_bounds__(256) void apr_adam_kernel(long long n, float *p, float *g, float *m, float *v, float *grad_out, int apply_update,
                                                       float step_size, float bc2s, float b1, float b2, float eps, const double *part,
                                                       int part_blocks, int used_blocks, int nb, float lam, int adv, double *losses)
{
    __shared__ double red[4];
    apr_adam_body(n, p, g, m, v, grad_out, apply_update, step_size, bc2s, b1, b2, eps, part, part_blocks, used_blocks, nb, lam, adv, losses,
                  blockIdx.x, gridDim.x, red);
}

// ---- host
template <bool GRAD>
static void apr_launch_rows(int regs, int grid, hipStream_t s, const AprStep &a)
{
    if (regs == 1) hipLaunchKernelGGL((apr_rows_kernel<GRAD, 1>), dim3(grid), dim3(256), 0, s, a);
    else if (regs == 2) hipLaunchKernelGGL((apr_rows_kernel<GRAD, 2>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((apr_rows_kernel<GRAD, 4>), dim3(grid), dim3(256), 0, s, a);
}

static int apr_limits(const char *who, int32_t U, int32_t I, int32_t dim, int64_t n, int32_t batch)
{
    if (U < 1 || I < 1) RK_FAIL(RK_EINVAL, "%s: an empty table (%d users, %d items)", who, U, I);
    if (dim < 1 || dim > RK_APR_MAX_DIM) RK_FAIL(RK_EINVAL, "%s: dim = %d, expected 1..%d", who, dim, RK_APR_MAX_DIM);
    if (batch < 1 || batch > RK_APR_MAX_BATCH) RK_FAIL(RK_EINVAL, "%s: batch = %d, expected 1..%d", who, batch, RK_APR_MAX_BATCH);
    if (n <= 0 || n >= (1LL << 31) / 3) RK_FAIL(RK_EINVAL, "%s: n = %lld, expected 1..%lld", who, (long long)n, (1LL << 31) / 3 - 1);
    if ((n + batch - 1) / batch >= (1LL << kAprStepBits) || (long long)U + I >= (1LL << kAprRowBits))
        RK_FAIL(RK_EINVAL, "%s: an epoch of < 2^20 steps and tables of < 2^24 rows are supported", who);
    return RK_OK;
}

static int apr_sort_bits(long long n_steps)
{
    int bits = kAprIncBits + kAprRowBits;
    while ((1LL << (bits - kAprIncBits - kAprRowBits)) < n_steps) ++bits;
    return bits;
}

RK_EXPORT int rk_apr_workspace(int32_t n_users, int32_t n_items, int32_t dim, int64_t n, int32_t batch, rk_apr_layout *out)
{
    if (!out) RK_FAIL(RK_EINVAL, "rk_apr_workspace: no layout to fill");
    int rc = apr_limits("rk_apr_workspace", n_users, n_items, dim, n, batch);
    if (rc) return rc;
    const long long n_steps = (n + batch - 1) / batch, nb = std::min<long long>(batch, n), T = 3 * nb, N = (long long)n_users + n_items;
    size_t sort_bytes = 0;
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                             (long long)(3 * n), 0, apr_sort_bits(n_steps), (hipStream_t) nullptr));
    rk_apr_layout L;
    memset(&L, 0, sizeof(L));
    int64_t at = 0;
    auto area = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 255) / 256 * 256 + 256; return o; };   // + a gap nothing writes
    L.run_stride = (int32_t)(T + 2);
    L.part_blocks = (int32_t)((nb + kAprTripletsPerBlock - 1) / kAprTripletsPerBlock);
    L.max_rows = (int32_t)T;
    L.n_steps = (int32_t)n_steps;
    L.keys = area(8 * 3 * n);
    L.keys_in = area(8 * 3 * n);
    L.sort_tmp_bytes = (int64_t)std::max<size_t>(sort_bytes, 16);
    L.sort_tmp = area(L.sort_tmp_bytes);
    L.run = area(4 * n_steps * L.run_stride);
    L.x = area(4 * nb);
    L.c = area(4 * nb);
    L.slot_of = area(4 * T);
    L.gamma = area(4 * T * dim);
    L.norm = area(4 * T);
    L.delta = area(4 * T * dim);
    L.x_adv = area(4 * nb);
    L.c_adv = area(4 * nb);
    L.part = area(8 * 3 * (int64_t)L.part_blocks);
    L.grad = area(4 * N * dim);
    L.bytes = at;
    *out = L;
    return RK_OK;
}

// what rk_apr_train_epoch refuses before it launches anything, and the layout of the epoch
static int apr_check_args(const char *who, const rk_apr_desc &D, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t n,
                          int32_t batch, int32_t adam_t0, int32_t apply_update, const double *losses, rk_apr_layout *L)
{
    if (!users || !pos || !neg || !losses) RK_FAIL(RK_EINVAL, "%s: a missing pointer", who);
    if (!D.table || !D.m || !D.v || !D.workspace) RK_FAIL(RK_EINVAL, "%s: a missing pointer in the descriptor", who);
    if (!apply_update && !D.grad) RK_FAIL(RK_EINVAL, "%s: apply_update = 0 needs desc.grad", who);
    if (!(D.eps >= 0.f) || !std::isfinite(D.eps) || !(D.adv_reg >= 0.f) || !std::isfinite(D.adv_reg))
        RK_FAIL(RK_EINVAL, "%s: eps and adv_reg must be finite and >= 0", who);
    if (adam_t0 < 0) RK_FAIL(RK_EINVAL, "%s: adam_t0 < 0", who);
    int rc = apr_limits(who, D.n_users, D.n_items, D.dim, n, batch);
    if (rc) return rc;
    rc = rk_apr_workspace(D.n_users, D.n_items, D.dim, n, batch, L);
    if (rc) return rc;
    if (D.workspace_bytes < L->bytes || (reinterpret_cast<uintptr_t>(D.workspace) & 255))
        RK_FAIL(RK_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (256-byte aligned)", who, (long long)D.workspace_bytes,
                (long long)L->bytes);
    return RK_OK;
}

static const char *const kAprRuleText[] = {"a user id outside [0, n_users)", "a positive item id outside [0, n_items)",
                                           "a negative item id outside [0, n_items)"};
static const char *apr_rule_text(int rule) { return kAprRuleText[rule >= RK_APR_BAD_USER && rule <= RK_APR_BAD_NEG ? rule - RK_APR_BAD_USER : 0]; }

RK_EXPORT int rk_apr_train_epoch(const rk_apr_desc *desc, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t n,
                                 int32_t batch, int32_t adam_t0, int32_t apply_update, double *losses, int32_t *status, void *stream)
{
    if (!desc || !status) RK_FAIL(RK_EINVAL, "rk_apr_train_epoch: a missing pointer");
    const rk_apr_desc &D = *desc;
    rk_apr_layout L;
    int rc = apr_check_args("rk_apr_train_epoch", D, users, pos, neg, n, batch, adam_t0, apply_update, losses, &L);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int U = D.n_users, d = D.dim, n_steps = L.n_steps;
    const long long N = (long long)D.n_users + D.n_items;

    {   // the ids first: nothing else is launched on a bad one
        RkScratch scratch(s);
        unsigned long long *first_bad = nullptr;
        RK_HIP(scratch.get(&first_bad, 1));
        RK_HIP(rk_first_bad_arm(first_bad, 1, s));
        hipLaunchKernelGGL(apr_check_kernel, dim3((int)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, s, users, pos, neg, (long long)n, U,
                           D.n_items, first_bad);
        RK_CHECK_LAUNCH();
        RK_HIP(rk_first_bad_status(first_bad, 1, status, s));
        int32_t h[2] = {0, 0};
        RK_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, s));
        RK_HIP(hipStreamSynchronize(s));
        if (h[0]) {
            RK_FAIL(RK_EINVAL, "rk_apr_train_epoch: rule %d (%s), first in triplet %d", h[0], apr_rule_text(h[0]), h[1]);
        }
    }

    char *ws = static_cast<char *>(D.workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + L.keys), *keys_in = reinterpret_cast<unsigned long long *>(ws + L.keys_in);
    int *run = reinterpret_cast<int *>(ws + L.run);
    float *gbuf = reinterpret_cast<float *>(ws + L.grad);
    double *part = reinterpret_cast<double *>(ws + L.part);

    // the plan, once per epoch
    hipLaunchKernelGGL(apr_keys_kernel, dim3((int)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, s, users, pos, neg, (long long)n, batch, U,
                       keys_in);
    RK_CHECK_LAUNCH();
    size_t sort_bytes = (size_t)L.sort_tmp_bytes;
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(ws + L.sort_tmp, sort_bytes, (const unsigned long long *)keys_in, keys, (long long)(3 * n), 0,
                                             apr_sort_bits(n_steps), s));
    hipLaunchKernelGGL(apr_runs_kernel, dim3(n_steps), dim3(256), 0, s, keys, (long long)n, batch, L.run_stride, run);
    RK_CHECK_LAUNCH();
    RK_HIP(rk_zero_async(gbuf, sizeof(float) * (size_t)N * d, s));

    const bool adv = D.adv_reg != 0.f;
    const bool vec4 = d == 64 && (reinterpret_cast<uintptr_t>(D.table) & 15) == 0;
    const long long nd = N * d;
    const int regs = (d + kWave - 1) / kWave;      // row elements a lane holds: 1, 2, or 4 (3 runs as 4)
    const int adam_grid = (int)std::max<long long>(1, std::min<long long>((nd + 255) / 256, 2048));
    for (int st = 0; st < n_steps; ++st) {
        const long long first = (long long)st * batch;
        const int nb = (int)std::min<long long>(batch, n - first);
        AprStep a;
        a.table = D.table;
        a.users = users + first; a.pos = pos + first; a.neg = neg + first;
        a.keys = keys + 3 * first;
        a.run = run + (size_t)st * L.run_stride;
        a.nb = nb; a.U = U; a.d = d;
        a.eps = D.eps; a.adv_reg = D.adv_reg; a.lam_b = D.lam / (float)nb;
        a.x = reinterpret_cast<float *>(ws + L.x); a.c = reinterpret_cast<float *>(ws + L.c);
        a.x_adv = reinterpret_cast<float *>(ws + L.x_adv); a.c_adv = reinterpret_cast<float *>(ws + L.c_adv);
        a.gamma = reinterpret_cast<float *>(ws + L.gamma); a.norm = reinterpret_cast<float *>(ws + L.norm);
        a.delta = reinterpret_cast<float *>(ws + L.delta); a.grad = gbuf;
        a.slot_of = reinterpret_cast<int *>(ws + L.slot_of);
        a.part = part; a.part_blocks = L.part_blocks;
        const int coef_grid = (nb + kAprTripletsPerBlock - 1) / kAprTripletsPerBlock, row_grid = (3 * nb + 3) / 4;
        if (vec4) hipLaunchKernelGGL((apr_coef_kernel<true, false>), dim3(coef_grid), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((apr_coef_kernel<false, false>), dim3(coef_grid), dim3(256), 0, s, a);
        RK_CHECK_LAUNCH();
        if (adv) {
            apr_launch_rows<false>(regs, row_grid, s, a);
            RK_CHECK_LAUNCH();
            if (vec4) hipLaunchKernelGGL((apr_coef_kernel<true, true>), dim3(coef_grid), dim3(256), 0, s, a);
            else hipLaunchKernelGGL((apr_coef_kernel<false, true>), dim3(coef_grid), dim3(256), 0, s, a);
            RK_CHECK_LAUNCH();
        }
        apr_launch_rows<true>(regs, row_grid, s, a);
        RK_CHECK_LAUNCH();
        const AdamCoef co = adam_coef(adam_t0 + st + 1, D.lr, D.beta1, D.beta2);
        hipLaunchKernelGGL(apr_adam_kernel, dim3(adam_grid), dim3(256), 0, s, nd, D.table, gbuf, D.m, D.v, D.grad, apply_update, co.step_size,
                           co.bc2s, D.beta1, D.beta2, D.adam_eps, part, L.part_blocks, coef_grid, nb, D.lam, adv ? 1 : 0, losses + 3 * (size_t)st);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}

// ---- a group of models in shared launches (rk_apr_train_epoch_group)
// What a member's steps have in common, written to the device once per epoch: `first` is the record of step 0 (a full step, or
// the only one), a later step moves its triplets, keys and run table on, and the last one has its own nb and fl(lam / nb).
struct AprMember {
    AprStep first;
    const AdamCoef *coef;                 // [n_steps]: adam_coef(adam_t0 + st + 1, ...) from the host
    float *p, *m, *v, *grad_out;
    double *losses;
    long long n, nd;
    int n_items, n_steps, batch, run_stride, nb_last, adam_grid, vec4, adv;
    float lam_b_last, lam, b1, b2, adam_eps;
};

// the member's record of step st; false when its epoch is over
__device__ __forceinline__ bool apr_member_step(const AprMember &M, const int st, AprStep &a)
{
    if (st >= M.n_steps) return false;
    a = M.first;
    const long long first = (long long)st * M.batch;
    a.users += first; a.pos += first; a.neg += first;
    a.keys += 3 * first;
    a.run += (size_t)st * M.run_stride;
    if (st == M.n_steps - 1) { a.nb = M.nb_last; a.lam_b = M.lam_b_last; }
    return true;
}

__global__ void apr_group_check_kernel(const AprMember *__restrict__ members, unsigned long long *__restrict__ first_bad)
{
    const AprMember &M = members[blockIdx.y];
    const int64_t *users = M.first.users, *pos = M.first.pos, *neg = M.first.neg;
    const int U = M.first.U, I = M.n_items;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < M.n; t += (long long)gridDim.x * blockDim.x) {
        const int64_t u = users[t], i = pos[t], j = neg[t];
        int rule = 0;
        if (u < 0 || u >= U) rule = RK_APR_BAD_USER;
        else if (i < 0 || i >= I) rule = RK_APR_BAD_POS;
        else if (j < 0 || j >= I) rule = RK_APR_BAD_NEG;
        if (rule) rk_record_bad(first_bad + blockIdx.y, t, rule);
    }
}

template <bool ADV>
__global__ __launch_bounds__(256) void apr_group_coef_kernel(const AprMember *__restrict__ members, int st)
{
    __shared__ double red[4];
    const AprMember &M = members[blockIdx.y];
    if (ADV && !M.adv) return;
    AprStep a;
    if (!apr_member_step(M, st, a)) return;
    if ((int)blockIdx.x * kAprTripletsPerBlock >= a.nb) return;
    if (M.vec4) apr_coef_body<true, ADV>(a, blockIdx.x, red);
    else apr_coef_body<false, ADV>(a, blockIdx.x, red);
}

template <bool GRAD, int REGS>
__global__ __launch_bounds__(256) void apr_group_rows_kernel(const AprMember *__restrict__ members, int st)
{
    const AprMember &M = members[blockIdx.y];
    if (!GRAD && !M.adv) return;
    AprStep a;
    if (!apr_member_step(M, st, a)) return;
    if ((int)blockIdx.x * 4 >= 3 * a.nb) return;
    apr_rows_body<GRAD, REGS>(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void apr_group_adam_kernel(const AprMember *__restrict__ members, int st, int apply_update)
{
    __shared__ double red[4];
    const AprMember &M = members[blockIdx.y];
    if (st >= M.n_steps || (int)blockIdx.x >= M.adam_grid) return;
    const int nb = st == M.n_steps - 1 ? M.nb_last : M.batch;
    const AdamCoef co = M.coef[st];
    apr_adam_body(M.nd, M.p, M.first.grad, M.m, M.v, M.grad_out, apply_update, co.step_size, co.bc2s, M.b1, M.b2,
                  M.adam_eps, M.first.part, M.first.part_blocks, (nb + kAprTripletsPerBlock - 1) / kAprTripletsPerBlock, nb, M.lam, M.adv,
                  M.losses + 3 * (size_t)st, blockIdx.x, M.adam_grid, red);
}

template <bool GRAD>
static void apr_group_launch_rows(int regs, dim3 grid, hipStream_t s, const AprMember *members, int st)
{
    if (regs == 1) hipLaunchKernelGGL((apr_group_rows_kernel<GRAD, 1>), grid, dim3(256), 0, s, members, st);
    else if (regs == 2) hipLaunchKernelGGL((apr_group_rows_kernel<GRAD, 2>), grid, dim3(256), 0, s, members, st);
    else hipLaunchKernelGGL((apr_group_rows_kernel<GRAD, 4>), grid, dim3(256), 0, s, members, st);
}

static bool apr_ranges_meet(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    if (!a || !b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

RK_EXPORT int rk_apr_train_epoch_group(int32_t n_rep, const rk_apr_desc *descs, const int64_t *const *users, const int64_t *const *pos,
                                       const int64_t *const *neg, const int64_t *n, int32_t batch, const int32_t *adam_t0,
                                       int32_t apply_update, double *const *losses, int32_t *status, void *stream)
{
    static const char *const who = "rk_apr_train_epoch_group";
    if (n_rep < 1 || n_rep > RK_APR_MAX_GROUP) RK_FAIL(RK_EINVAL, "%s: n_rep = %d, expected 1..%d", who, n_rep, RK_APR_MAX_GROUP);
    if (!descs || !users || !pos || !neg || !n || !adam_t0 || !losses || !status) RK_FAIL(RK_EINVAL, "%s: a missing array", who);
    rk_apr_layout L[RK_APR_MAX_GROUP];
    for (int r = 0; r < n_rep; ++r) {
        if (descs[r].dim != descs[0].dim) RK_FAIL(RK_EINVAL, "%s: member %d has dim = %d, member 0 has %d", who, r, descs[r].dim, descs[0].dim);
        const int rc = apr_check_args(who, descs[r], users[r], pos[r], neg[r], n[r], batch, adam_t0[r], apply_update, losses[r], &L[r]);
        if (rc) {
            char text[sizeof(rk_err_buf)];
            snprintf(text, sizeof(text), "%s", rk_err_buf);
            RK_FAIL(rc, "member %d: %s", r, text);
        }
    }
    for (int r = 0; r < n_rep; ++r) {
        const rk_apr_desc &A = descs[r];
        const int64_t a_bytes = 4 * ((int64_t)A.n_users + A.n_items) * A.dim;
        const void *pa[5] = {A.table, A.m, A.v, A.grad, A.workspace};
        const int64_t na[5] = {a_bytes, a_bytes, a_bytes, a_bytes, L[r].bytes};
        for (int q = 0; q < r; ++q) {
            const rk_apr_desc &B = descs[q];
            const int64_t b_bytes = 4 * ((int64_t)B.n_users + B.n_items) * B.dim;
            const void *pb[5] = {B.table, B.m, B.v, B.grad, B.workspace};
            const int64_t nbq[5] = {b_bytes, b_bytes, b_bytes, b_bytes, L[q].bytes};
            for (int x = 0; x < 5; ++x)
                for (int y = 0; y < 5; ++y)
                    if (apr_ranges_meet(pa[x], na[x], pb[y], nbq[y]))
                        RK_FAIL(RK_EINVAL, "%s: members %d and %d share bytes of their tables, moments, gradients or workspaces", who, q, r);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const int d = descs[0].dim;

    // the members' table and the Adam coefficients of every (member, step), built on the host
    std::vector<AprMember> mem((size_t)n_rep);
    std::vector<AdamCoef> coef;
    std::vector<size_t> coef_at((size_t)n_rep);
    int max_steps = 0;
    long long max_n = 0;
    bool any_adv = false;
    for (int r = 0; r < n_rep; ++r) {
        const rk_apr_desc &D = descs[r];
        const rk_apr_layout &l = L[r];
        char *ws = static_cast<char *>(D.workspace);
        const long long first_last = (long long)(l.n_steps - 1) * batch;
        AprMember &M = mem[(size_t)r];
        memset(&M, 0, sizeof(M));
        AprStep &a = M.first;
        a.table = D.table;
        a.users = users[r]; a.pos = pos[r]; a.neg = neg[r];
        a.keys = reinterpret_cast<unsigned long long *>(ws + l.keys);
        a.run = reinterpret_cast<int *>(ws + l.run);
        a.nb = (int)std::min<long long>(batch, n[r]); a.U = D.n_users; a.d = d;
        a.eps = D.eps; a.adv_reg = D.adv_reg; a.lam_b = D.lam / (float)a.nb;
        a.x = reinterpret_cast<float *>(ws + l.x); a.c = reinterpret_cast<float *>(ws + l.c);
        a.x_adv = reinterpret_cast<float *>(ws + l.x_adv); a.c_adv = reinterpret_cast<float *>(ws + l.c_adv);
        a.gamma = reinterpret_cast<float *>(ws + l.gamma); a.norm = reinterpret_cast<float *>(ws + l.norm);
        a.delta = reinterpret_cast<float *>(ws + l.delta); a.grad = reinterpret_cast<float *>(ws + l.grad);
        a.slot_of = reinterpret_cast<int *>(ws + l.slot_of);
        a.part = reinterpret_cast<double *>(ws + l.part); a.part_blocks = l.part_blocks;
        M.p = D.table; M.m = D.m; M.v = D.v; M.grad_out = D.grad;
        M.losses = losses[r];
        M.n = n[r];
        M.nd = ((long long)D.n_users + D.n_items) * d;
        M.n_items = D.n_items; M.n_steps = l.n_steps; M.batch = batch; M.run_stride = l.run_stride;
        M.nb_last = (int)(n[r] - first_last);
        M.adam_grid = (int)std::max<long long>(1, std::min<long long>((M.nd + 255) / 256, 2048));
        M.vec4 = d == 64 && (reinterpret_cast<uintptr_t>(D.table) & 15) == 0;
        M.adv = D.adv_reg != 0.f;
        M.lam_b_last = D.lam / (float)M.nb_last;
        M.lam = D.lam; M.b1 = D.beta1; M.b2 = D.beta2; M.adam_eps = D.adam_eps;
        coef_at[(size_t)r] = coef.size();
        for (int st = 0; st < l.n_steps; ++st) coef.push_back(adam_coef(adam_t0[r] + st + 1, D.lr, D.beta1, D.beta2));
        max_steps = std::max(max_steps, (int)l.n_steps);
        max_n = std::max<long long>(max_n, n[r]);
        any_adv = any_adv || M.adv;
    }

    RkScratch scratch(s);
    AprMember *d_mem = nullptr;
    AdamCoef *d_coef = nullptr;
    unsigned long long *first_bad = nullptr;
    RK_HIP(scratch.get(&d_mem, (size_t)n_rep));
    RK_HIP(scratch.get(&d_coef, coef.size()));
    RK_HIP(scratch.get(&first_bad, (size_t)n_rep));
    for (int r = 0; r < n_rep; ++r) mem[(size_t)r].coef = d_coef + coef_at[(size_t)r];
    // the two uploads are over when the synchronisation below returns, so the host copies may go when this function does
    RK_HIP(hipMemcpyAsync(d_mem, mem.data(), sizeof(AprMember) * (size_t)n_rep, hipMemcpyHostToDevice, s));
    RK_HIP(hipMemcpyAsync(d_coef, coef.data(), sizeof(AdamCoef) * coef.size(), hipMemcpyHostToDevice, s));

    {   // the ids of all members first: nothing else is launched on a bad one
        RK_HIP(rk_first_bad_arm(first_bad, (int)n_rep, s));
        hipLaunchKernelGGL(apr_group_check_kernel, dim3((int)std::min<long long>((max_n + 255) / 256, 4096), n_rep), dim3(256), 0, s, d_mem, first_bad);
        RK_CHECK_LAUNCH();
        RK_HIP(rk_first_bad_status(first_bad, (int)n_rep, status, s));
        int32_t h[2 * RK_APR_MAX_GROUP];
        RK_HIP(hipMemcpyAsync(h, status, sizeof(int32_t) * 2 * (size_t)n_rep, hipMemcpyDeviceToHost, s));
        RK_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < n_rep; ++r)
            if (h[2 * r])
                RK_FAIL(RK_EINVAL, "%s: member %d: rule %d (%s), first in triplet %d", who, r, h[2 * r], apr_rule_text(h[2 * r]), h[2 * r + 1]);
    }

    // every member's plan, once per epoch
    for (int r = 0; r < n_rep; ++r) {
        const rk_apr_desc &D = descs[r];
        const rk_apr_layout &l = L[r];
        char *ws = static_cast<char *>(D.workspace);
        unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + l.keys), *keys_in = reinterpret_cast<unsigned long long *>(ws + l.keys_in);
        hipLaunchKernelGGL(apr_keys_kernel, dim3((int)std::min<long long>((n[r] + 255) / 256, 4096)), dim3(256), 0, s, users[r], pos[r], neg[r],
                           (long long)n[r], batch, D.n_users, keys_in);
        RK_CHECK_LAUNCH();
        size_t sort_bytes = (size_t)l.sort_tmp_bytes;
        RK_HIP(hipcub::DeviceRadixSort::SortKeys(ws + l.sort_tmp, sort_bytes, (const unsigned long long *)keys_in, keys, (long long)(3 * n[r]), 0,
                                                 apr_sort_bits(l.n_steps), s));
        hipLaunchKernelGGL(apr_runs_kernel, dim3(l.n_steps), dim3(256), 0, s, keys, (long long)n[r], batch, l.run_stride, reinterpret_cast<int *>(ws + l.run));
        RK_CHECK_LAUNCH();
        RK_HIP(rk_zero_async(ws + l.grad, sizeof(float) * (size_t)mem[(size_t)r].nd, s));
    }

    const int regs = (d + kWave - 1) / kWave;
    for (int st = 0; st < max_steps; ++st) {
        int nb_max = 0, adam_max = 0;          // the widest grids among the members that still have a step st
        for (int r = 0; r < n_rep; ++r) {
            const AprMember &M = mem[(size_t)r];
            if (st >= M.n_steps) continue;
            nb_max = std::max(nb_max, st == M.n_steps - 1 ? M.nb_last : batch);
            adam_max = std::max(adam_max, M.adam_grid);
        }
        const dim3 coef_grid((nb_max + kAprTripletsPerBlock - 1) / kAprTripletsPerBlock, n_rep), row_grid((3 * nb_max + 3) / 4, n_rep);
        hipLaunchKernelGGL((apr_group_coef_kernel<false>), coef_grid, dim3(256), 0, s, d_mem, st);
        RK_CHECK_LAUNCH();
        if (any_adv) {
            apr_group_launch_rows<false>(regs, row_grid, s, d_mem, st);
            RK_CHECK_LAUNCH();
            hipLaunchKernelGGL((apr_group_coef_kernel<true>), coef_grid, dim3(256), 0, s, d_mem, st);
            RK_CHECK_LAUNCH();
        }
        apr_group_launch_rows<true>(regs, row_grid, s, d_mem, st);
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(apr_group_adam_kernel, dim3(adam_max, n_rep), dim3(256), 0, s, d_mem, st, (int)apply_update);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}
