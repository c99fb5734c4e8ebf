// Mult-VAE victim (Liang, Krishnan, Hoffman and Jebara, WWW 2018): a multinomial variational autoencoder over the catalogue;
// include/recad_hip.h states the definition.  A step is a dense B x I problem: a sparse input layer that gathers rows of W1,
// nine products through the fp32 MFMA GEMM (whole-K: each result is the k-ordered fmaf chain), one fused pass per logits row
// (maximum, log-sum-exp, loss, gradient in place), an item-grouped walk for the input layer's gradient, and one Adam pass over
// the flat parameter buffer.  Nothing here adds floats atomically: the kept entries of a step are sorted once by (item, batch
// position), every reduction has a fixed order, and the same call gives the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "gemm.h"

// pre1, the tanh backwards and the bias sums round every operation on its own; where the definition asks for a fused
// multiply-add the code says fmaf
#pragma clang fp contract(off)

static constexpr int kMvPosBits = 12;                         // a batch position in the low bits of a sort key
static constexpr unsigned long long kMvHashMul = 0xD1342543DE82EF95ULL, kMvEpsStream = 0xA5A5A5A5A5A5A5A5ULL;
static_assert(RK_MVAE_MAX_BATCH == (1 << kMvPosBits), "a batch position must fit the key's low bits");

// ---- validation: reads the ids and the rating rows only.  First offending (row, rule) by rk_record_bad;
// rows_too (training) also walks each row and adds its length to its step's count (integer atomics).
__global__ void mv_check_kernel(const int *__restrict__ ids, long long n, int U, int I, const int *__restrict__ rowptr,
                                const int *__restrict__ col, int rows_too, int batch, unsigned long long *__restrict__ step_nnz,
                                unsigned long long *__restrict__ first_bad)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const int u = ids[t];
        int rule = 0;
        if (u < 0 || u >= U) rule = RK_MVAE_BAD_USER;
        else if (rows_too) {
            const int b = rowptr[u], e = rowptr[u + 1];
            if (e <= b) rule = RK_MVAE_EMPTY_ROW;
            else {
                int prev = -1;
                for (int k = b; k < e; ++k) {
                    const int c = col[k];
                    if (c <= prev || c >= I) { rule = RK_MVAE_BAD_ROW; break; }
                    prev = c;
                }
                if (!rule) atomicAdd(step_nnz + t / batch, (unsigned long long)(e - b));
            }
        }
        if (rule) rk_record_bad(first_bad, t, rule);
    }
}

// not rk_first_bad_status_kernel: a clean first_bad word is followed by the steps' counts against nnz_cap
__global__ void mv_status_kernel(const unsigned long long *__restrict__ first_bad, const unsigned long long *__restrict__ step_nnz,
                                 int n_steps, long long nnz_cap, int *__restrict__ status)
{
    const unsigned long long k = *first_bad;
    if (k != ~0ULL) { status[0] = (int)(k & 31ULL); status[1] = (int)(k >> 5); return; }
    for (int s = 0; s < n_steps; ++s)
        if ((long long)step_nnz[s] > nnz_cap) { status[0] = RK_MVAE_NNZ_CAP; status[1] = s; return; }
    status[0] = 0; status[1] = -1;
}

// ---- step 1: brp = the prefix sums of the step's row lengths, c_u = n_u^-1/2 / keep in double, rounded once (0 for an
// empty row, which only inference lets through).  One workgroup.
__global__ __launch_bounds__(256) void mv_prep_kernel(const int *__restrict__ ids, int nb, const int *__restrict__ rowptr, double keep,
                                                      int *__restrict__ brp, float *__restrict__ c)
{
    __shared__ int part[256];
    const int per = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    int s = 0;
    for (int b = lo; b < hi; ++b) {
        const int u = ids[b], len = rowptr[u + 1] - rowptr[u];
        s += len;
        c[b] = len > 0 ? (float)(1.0 / sqrt((double)len) / keep) : 0.f;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int t = part[i]; part[i] = run; run += t; }
        brp[nb] = run;
    }
    __syncthreads();
    int at = part[threadIdx.x];
    for (int b = lo; b < hi; ++b) {
        const int u = ids[b];
        brp[b] = at;
        at += rowptr[u + 1] - rowptr[u];
    }
}

// the keep decision of every entry of the step and its sort key: item << 12 | batch position when kept, n_items << 12 when
// dropped (those sort behind every item).  One workgroup per batch row.
__global__ __launch_bounds__(256) void mv_mask_kernel(const int *__restrict__ ids, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      const int *__restrict__ brp, int I, unsigned long long seed_step, unsigned thresh24,
                                                      int *__restrict__ keep, unsigned long long *__restrict__ keys)
{
    const int b = blockIdx.x, u = ids[b], beg = rowptr[u], len = rowptr[u + 1] - beg, at = brp[b];
    const unsigned long long seed_u = rk_drop_step_seed(seed_step, (unsigned long long)u);
    for (int k = threadIdx.x; k < len; k += 256) {
        const int i = col[beg + k];
        const bool kp = rk_drop_keep(seed_u, (unsigned)i, thresh24);
        keep[at + k] = kp ? 1 : 0;
        keys[at + k] = kp ? (((unsigned long long)i << kMvPosBits) | (unsigned long long)b) : ((unsigned long long)I << kMvPosBits);
    }
}

// the item-grouped view of the kept entries: t_ptr[i] = first sorted key of an item >= i (t_ptr[I] = the kept count),
// t_row = the batch positions, ascending inside an item
__global__ void mv_tptr_kernel(int I, int nnz, const unsigned long long *__restrict__ keys, int *__restrict__ t_ptr)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > I) return;
    int lo = 0, hi = nnz;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)(keys[mid] >> kMvPosBits) < c) lo = mid + 1; else hi = mid;
    }
    t_ptr[c] = lo;
}

__global__ void mv_trow_kernel(int nnz, const unsigned long long *__restrict__ keys, int *__restrict__ t_row)
{
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += gridDim.x * blockDim.x)
        t_row[e] = (int)(keys[e] & ((1ULL << kMvPosBits) - 1ULL));
}

// ---- step 2: the sparse layer.  Workgroup (b, y) holds elements h = 256 y + thread of row b and adds the kept rows of W1 in
// ascending item order: the loads of a wave are consecutive floats of one W1 row.  The row is taken 256 entries at a time: the
// kept item ids are compacted into LDS in order (ballot and popcount), then every thread issues eight row loads before it adds
// them one after the other, so the chain of dependent adds does not wait for one load at a time (the first form, one guarded load
// per add, spent 193 us of a 960 us step at the ml1m shape).  keep == NULL: every entry counts (inference).
__global__ __launch_bounds__(256) void mv_sparse_kernel(const int *__restrict__ ids, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        const int *__restrict__ brp, const int *__restrict__ keep, const float *__restrict__ c,
                                                        const float *__restrict__ W1, const float *__restrict__ b1, int H, float *__restrict__ a,
                                                        float *__restrict__ pre1, float *__restrict__ h1)
{
    __shared__ int items[256];
    __shared__ int wave_cnt[4];
    const int b = blockIdx.x, h = blockIdx.y * 256 + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = h < H;                     // threads past H still help to stage the ids: no early return before the barriers
    const int u = ids[b], beg = rowptr[u], len = rowptr[u + 1] - beg;
    const int *kp = keep ? keep + brp[b] : nullptr;
    float acc = 0.f;
    for (int base = 0; base < len; base += 256) {
        const int k = base + (int)threadIdx.x;
        const bool on = k < len && (!kp || kp[k]);
        const int it = on ? col[beg + k] : 0;
        const unsigned long long mask = __ballot(on);
        if (lane == 0) wave_cnt[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { if (q < w) before += wave_cnt[q]; total += wave_cnt[q]; }
        if (on) items[before + __popcll(mask & ((1ULL << lane) - 1ULL))] = it;
        __syncthreads();
        if (live) {
            int j = 0;
            for (; j + 8 <= total; j += 8) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = W1[(size_t)items[j + q] * H + h];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = acc + v[q];
            }
            for (; j < total; ++j) acc = acc + W1[(size_t)items[j] * H + h];
        }
        __syncthreads();                         // items and wave_cnt are rewritten by the next 256 entries
    }
    if (!live) return;
    float p = c[b] * acc;
    p = p + b1[h];
    const size_t o = (size_t)b * H + h;
    a[o] = acc;
    pre1[o] = p;
    h1[o] = (float)tanh((double)p);
}

__global__ void mv_tanh_kernel(long long n, const float *__restrict__ pre, float *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (float)tanh((double)pre[i]);
}

// dp = dh * (1 - h * h), three roundings
__global__ void mv_tanh_bwd_kernel(long long n, const float *__restrict__ dh, const float *__restrict__ h, float *__restrict__ dp)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float t = h[i] * h[i];
        const float s = 1.f - t;
        dp[i] = dh[i] * s;
    }
}

// ---- step 4: eps, z and KL.  One wave per row; the KL sum meets in the wave's fixed butterfly.
__global__ __launch_bounds__(256) void mv_sample_kernel(const int *__restrict__ ids, int nb, int L, const float *__restrict__ ml,
                                                        unsigned long long eps_seed_step, float *__restrict__ eps, float *__restrict__ z,
                                                        double *__restrict__ kl)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nb) return;
    const unsigned long long su = rk_drop_step_seed(eps_seed_step, (unsigned long long)ids[row]);
    const float *mu = ml + (size_t)row * 2 * L, *lv = mu + L;
    double s = 0.0;
    for (int j = lane; j < L; j += 64) {
        const unsigned long long r1 = rk_mix64(su ^ ((unsigned long long)(2 * j) * kMvHashMul));
        const unsigned long long r2 = rk_mix64(su ^ ((unsigned long long)(2 * j + 1) * kMvHashMul));
        const double u1 = (double)((r1 >> 11) + 1ULL) * 0x1p-53, u2 = (double)(r2 >> 11) * 0x1p-53;
        const float e = (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
        const double m = mu[j], v = lv[j];
        eps[(size_t)row * L + j] = e;
        z[(size_t)row * L + j] = (float)(m + (double)e * exp(0.5 * v));
        s += ((1.0 + v) - m * m) - exp(v);
    }
    s = wave_sum(s);
    if (lane == 0) kl[row] = -0.5 * s;
}

// dmu and dlogvar into dml = [dmu | dlogvar], in double and rounded once; cb = beta / B, cb2 = beta / 2B
__global__ void mv_sample_bwd_kernel(int nb, int L, const float *__restrict__ dz, const float *__restrict__ ml, const float *__restrict__ eps,
                                     double cb, double cb2, float *__restrict__ dml)
{
    const long long n = (long long)nb * L;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
        const long long r = q / L;
        const int j = (int)(q - r * L);
        const double g = dz[q], m = ml[r * 2 * L + j], v = ml[r * 2 * L + L + j], e = eps[q];
        dml[r * 2 * L + j] = (float)(g + cb * m);
        dml[r * 2 * L + L + j] = (float)(0.5 * g * e * exp(0.5 * v) + cb2 * (exp(v) - 1.0));
    }
}

// ---- step 6: one workgroup per logits row.  The row's items are marked in an LDS bitmap (integer atomics), then three
// passes over the row: the maximum, sum exp(l - max) in double (a fixed tree), and dl written over the logits with nll.
template <typename T>
__device__ __forceinline__ T mv_block_max(T v, T *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = red[0];
    for (int q = 1; q < 4; ++q) t = red[q] > t ? red[q] : t;
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void mv_row_kernel(const int *__restrict__ ids, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                     int I, int nb, float *__restrict__ logits, double *__restrict__ lse_out,
                                                     double *__restrict__ nll_out)
{
    extern __shared__ unsigned mv_bits[];
    __shared__ double red[4];
    __shared__ float redf[4];
    const int b = blockIdx.x, u = ids[b], beg = rowptr[u], len = rowptr[u + 1] - beg, words = (I + 31) >> 5;
    float *row = logits + (size_t)b * I;
    for (int w = threadIdx.x; w < words; w += 256) mv_bits[w] = 0u;
    __syncthreads();
    for (int k = threadIdx.x; k < len; k += 256) {
        const int i = col[beg + k];
        atomicOr(&mv_bits[i >> 5], 1u << (i & 31));
    }
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < I; i += 256) mx = fmaxf(mx, row[i]);
    mx = mv_block_max(mx, redf);            // (its barriers also publish the bitmap)
    double s = 0.0;
    for (int i = threadIdx.x; i < I; i += 256) s += exp((double)row[i] - (double)mx);
    s = block_sum_256(s, red);
    const double lse = (double)mx + log(s), dn = (double)len, dB = (double)nb;
    double nll = 0.0;
    for (int i = threadIdx.x; i < I; i += 256) {
        const double l = row[i];
        const bool x = (mv_bits[i >> 5] >> (i & 31)) & 1u;
        row[i] = (float)((dn * exp(l - lse) - (x ? 1.0 : 0.0)) / dB);
        if (x) nll += lse - l;
    }
    nll = block_sum_256(nll, red);
    if (threadIdx.x == 0) { lse_out[b] = lse; nll_out[b] = nll; }
}

// dst[c] = sum over the rows of src[r, c], fp32 adds in ascending r; a wave reads consecutive columns
__global__ void mv_colsum_kernel(int rows, int cols, const float *__restrict__ src, float *__restrict__ dst)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) s = s + src[(size_t)r * cols + c];
    dst[c] = s;
}

// ---- gW1: workgroup (i, y) walks the batch rows that hold item i as a kept entry, in ascending batch position; thread h reads
// consecutive floats of dp1's row.  An item without kept entries gets +0.0.
__global__ __launch_bounds__(256) void mv_gw1_kernel(const int *__restrict__ t_ptr, const int *__restrict__ t_row, const float *__restrict__ c,
                                                     const float *__restrict__ dp1, int H, float *__restrict__ gW1)
{
    const int i = blockIdx.x, h = blockIdx.y * 256 + threadIdx.x;
    if (h >= H) return;
    const int beg = t_ptr[i], end = t_ptr[i + 1];
    float acc = 0.f;
    for (int k = beg; k < end; ++k) {
        const int r = t_row[k];
        acc = fmaf(c[r], dp1[(size_t)r * H + h], acc);
    }
    gW1[(size_t)i * H + h] = acc;
}

// ---- step 8: Adam over the flat buffer (copies the gradient out when asked, updates when asked).  Workgroup 0 also adds the
// rows' nll and KL in a fixed order: losses = {loss, mean nll, mean KL}.
__global__ __launch_bounds__(256) void mv_adam_kernel(long long n, float *p, const float *g, float *m, float *v, float *grad_out, int apply_update,
                                                      float step_size, float bc2s, float b2, float w1, float w2, float eps, const double *nll,
                                                      const double *kl, int nb, double beta, double *losses)
{
    __shared__ double red[4];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float gi = g[i];
        if (grad_out) grad_out[i] = gi;
        if (apply_update) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_elem(pp, mm, vv, gi, w1, b2, w2, step_size, bc2s, eps);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
    if (blockIdx.x != 0) return;
    double a = 0.0, k = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) { a += nll[i]; k += kl[i]; }
    a = block_sum_256(a, red);
    k = block_sum_256(k, red);
    if (threadIdx.x == 0) {
        losses[0] = (a + beta * k) / (double)nb;
        losses[1] = a / (double)nb;
        losses[2] = k / (double)nb;
    }
}

// out[q] = chain_k fmaf(h2[q, k], W4[item_q, k]) + b4[item_q]: the GEMM's order, so a pair equals the matrix entry to the bit
__global__ void mv_pair_kernel(int n, int H, const float *__restrict__ h2, const int *__restrict__ items, const float *__restrict__ W4,
                               const float *__restrict__ b4, float *__restrict__ out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int i = items[q];
    const float *x = h2 + (size_t)q * H, *w = W4 + (size_t)i * H;
    float s = 0.f;
    for (int k = 0; k < H; ++k) s = fmaf(x[k], w[k], s);
    out[q] = s + b4[i];
}

__global__ void mv_items_check_kernel(const int *__restrict__ items, long long n, int I, unsigned long long *__restrict__ first_bad)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x)
        if (items[t] < 0 || items[t] >= I) rk_record_bad(first_bad, t, RK_MVAE_BAD_ITEM);
}

// ---- host
static int mv_gemm(hipStream_t s, int M, int N, int K, const float *A, long long a_rs, long long a_cs, const float *B, long long b_rs,
                   long long b_cs, float *C, int ldc, const float *bias)
{
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.split_k = 1;
    g.M = M; g.N = N; g.K = K; g.A = A; g.a_rs = a_rs; g.a_cs = a_cs; g.B = B; g.b_rs = b_rs; g.b_cs = b_cs;
    g.C = C; g.ldc = ldc; g.col_bias = bias;
    RK_HIP(gemm_f32_launch(g, s));
    return RK_OK;
}

static inline int mv_grid(long long n, int cap = 2048) { return (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap)); }

static int mv_limits(const char *who, int32_t I, int32_t H, int32_t L, int32_t batch, int64_t nnz_cap)
{
    if (I < 1 || I > RK_MVAE_MAX_ITEMS) RK_FAIL(RK_EINVAL, "%s: n_items = %d, expected 1..%d", who, I, RK_MVAE_MAX_ITEMS);
    if (H < 1 || H > RK_MVAE_MAX_HIDDEN) RK_FAIL(RK_EINVAL, "%s: hidden = %d, expected 1..%d", who, H, RK_MVAE_MAX_HIDDEN);
    if (L < 1 || L > RK_MVAE_MAX_LATENT) RK_FAIL(RK_EINVAL, "%s: latent = %d, expected 1..%d", who, L, RK_MVAE_MAX_LATENT);
    if (batch < 1 || batch > RK_MVAE_MAX_BATCH) RK_FAIL(RK_EINVAL, "%s: batch = %d, expected 1..%d", who, batch, RK_MVAE_MAX_BATCH);
    if (nnz_cap < 1 || nnz_cap >= (1LL << 31)) RK_FAIL(RK_EINVAL, "%s: nnz_cap = %lld, expected 1..2^31 - 1", who, (long long)nnz_cap);
    return RK_OK;
}

static int mv_sort_bits(int I)
{
    int bits = kMvPosBits + 1;
    while ((1LL << (bits - kMvPosBits)) <= (long long)I) ++bits;     // the dropped entries' key is I itself
    return bits;
}

RK_EXPORT int rk_mvae_workspace(int32_t n_items, int32_t hidden, int32_t latent, int32_t batch, int64_t nnz_cap, rk_mvae_layout *out)
{
    if (!out) RK_FAIL(RK_EINVAL, "rk_mvae_workspace: no layout to fill");
    int rc = mv_limits("rk_mvae_workspace", n_items, hidden, latent, batch, nnz_cap);
    if (rc) return rc;
    const int64_t I = n_items, H = hidden, L = latent, B = batch;
    rk_mvae_layout Y;
    memset(&Y, 0, sizeof(Y));
    int64_t at = 0;
    auto area = [&at](int64_t bytes) { const int64_t o = at; at += (bytes + 255) / 256 * 256 + 256; return o; };   // + a gap nothing writes
    Y.batch = batch; Y.nnz_cap = nnz_cap;
    Y.brp = area(4 * (B + 1));
    Y.keep = area(4 * nnz_cap);
    Y.keys = area(8 * nnz_cap);
    Y.keys_in = area(8 * nnz_cap);
    Y.t_ptr = area(4 * (I + 1));
    Y.t_row = area(4 * nnz_cap);
    Y.c = area(4 * B);
    Y.a = area(4 * B * H); Y.pre1 = area(4 * B * H); Y.h1 = area(4 * B * H);
    Y.ml = area(4 * B * 2 * L); Y.eps = area(4 * B * L); Y.z = area(4 * B * L); Y.kl = area(8 * B);
    Y.pre2 = area(4 * B * H); Y.h2 = area(4 * B * H);
    Y.logits = area(4 * B * I); Y.lse = area(8 * B); Y.nll = area(8 * B);
    Y.dh2 = area(4 * B * H); Y.dp2 = area(4 * B * H); Y.dz = area(4 * B * L); Y.dml = area(4 * B * 2 * L);
    Y.dh1 = area(4 * B * H); Y.dp1 = area(4 * B * H);
    int64_t p = 0;
    Y.w1 = p; p += I * H; Y.b1 = p; p += H; Y.w2 = p; p += 2 * L * H; Y.b2 = p; p += 2 * L; Y.w3 = p; p += H * L; Y.b3 = p; p += H;
    Y.w4 = p; p += I * H; Y.b4 = p; p += I;
    Y.n_params = p;
    Y.grad = area(4 * p);
    Y.bytes = at;
    *out = Y;
    return RK_OK;
}

// the descriptor's checks that every entry shares; fills the layout the workspace was made for
static int mv_open(const char *who, const rk_mvae_desc &D, rk_mvae_layout *Y)
{
    if (!D.rowptr || !D.col || !D.params || !D.workspace) RK_FAIL(RK_EINVAL, "%s: a missing pointer in the descriptor", who);
    if (D.n_users < 1) RK_FAIL(RK_EINVAL, "%s: n_users = %d", who, D.n_users);
    int rc = mv_limits(who, D.n_items, D.hidden, D.latent, D.ws_batch, D.ws_nnz_cap);
    if (rc) return rc;
    rc = rk_mvae_workspace(D.n_items, D.hidden, D.latent, D.ws_batch, D.ws_nnz_cap, Y);
    if (rc) return rc;
    if (D.workspace_bytes < Y->bytes || (reinterpret_cast<uintptr_t>(D.workspace) & 255))
        RK_FAIL(RK_EINVAL, "%s: the workspace has %lld bytes, %lld are needed (256-byte aligned)", who, (long long)D.workspace_bytes, (long long)Y->bytes);
    return RK_OK;
}

// runs the id check and reads its answer back (the entry's only synchronisation); step_nnz_host: the steps' entry counts
static int mv_check_ids(const char *who, const rk_mvae_desc &D, const int32_t *ids, int64_t n, int rows_too, int batch, int n_steps, const int32_t *items,
                        int32_t *status, std::vector<unsigned long long> *step_nnz_host, hipStream_t s)
{
    RkScratch scratch(s);
    unsigned long long *dev = nullptr;       // [0] = first_bad, [1 ..] = the steps' counts
    int32_t *st = status;
    RK_HIP(scratch.get(&dev, (size_t)n_steps + 1));
    if (!st) RK_HIP(scratch.get(&st, 2));
    RK_HIP(hipMemsetAsync(dev, 0xff, sizeof(unsigned long long), s));
    RK_HIP(hipMemsetAsync(dev + 1, 0, sizeof(unsigned long long) * (size_t)n_steps, s));
    hipLaunchKernelGGL(mv_check_kernel, dim3(mv_grid(n, 4096)), dim3(256), 0, s, ids, (long long)n, D.n_users, D.n_items, D.rowptr, D.col, rows_too, batch,
                       dev + 1, dev);
    RK_CHECK_LAUNCH();
    if (items) {
        hipLaunchKernelGGL(mv_items_check_kernel, dim3(mv_grid(n, 4096)), dim3(256), 0, s, items, (long long)n, D.n_items, dev);
        RK_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mv_status_kernel, dim3(1), dim3(1), 0, s, dev, dev + 1, n_steps, rows_too ? (long long)D.ws_nnz_cap : (1LL << 62), st);
    RK_CHECK_LAUNCH();
    int32_t h[2] = {0, 0};
    RK_HIP(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, s));
    if (step_nnz_host) {
        step_nnz_host->assign((size_t)n_steps, 0ULL);
        RK_HIP(hipMemcpyAsync(step_nnz_host->data(), dev + 1, sizeof(unsigned long long) * (size_t)n_steps, hipMemcpyDeviceToHost, s));
    }
    RK_HIP(hipStreamSynchronize(s));
    if (h[0]) {
        static const char *const what[] = {"a user id outside [0, n_users)", "a row whose item ids are not strictly ascending inside [0, n_items)",
                                           "a user without a train item", "a step with more entries than nnz_cap", "an item id outside [0, n_items)"};
        RK_FAIL(RK_EINVAL, "%s: rule %d (%s), first at %d", who, h[0], what[h[0] >= RK_MVAE_BAD_USER && h[0] <= RK_MVAE_BAD_ITEM ? h[0] - RK_MVAE_BAD_USER : 0],
                h[1]);
    }
    return RK_OK;
}

struct MvPtr {
    float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
    MvPtr(float *base, const rk_mvae_layout &Y)
        : W1(base + Y.w1), b1(base + Y.b1), W2(base + Y.w2), b2(base + Y.b2), W3(base + Y.w3), b3(base + Y.b3), W4(base + Y.w4), b4(base + Y.b4) {}
};

// inference up to h2 for nb <= ws_batch users: no dropout, z = mu (only the first L rows of W2 are multiplied; mu lies in
// the ml area with row stride L)
static int mv_infer_h2(const rk_mvae_desc &D, const rk_mvae_layout &Y, const int32_t *ids, int nb, hipStream_t s)
{
    char *ws = static_cast<char *>(D.workspace);
    const int H = D.hidden, L = D.latent;
    const MvPtr P(D.params, Y);
    auto F = [ws](int64_t o) { return reinterpret_cast<float *>(ws + o); };
    hipLaunchKernelGGL(mv_prep_kernel, dim3(1), dim3(256), 0, s, ids, nb, D.rowptr, 1.0, reinterpret_cast<int *>(ws + Y.brp), F(Y.c));
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(mv_sparse_kernel, dim3(nb, (H + 255) / 256), dim3(256), 0, s, ids, D.rowptr, D.col, (const int *)nullptr, (const int *)nullptr,
                       (const float *)F(Y.c), (const float *)P.W1, (const float *)P.b1, H, F(Y.a), F(Y.pre1), F(Y.h1));
    RK_CHECK_LAUNCH();
    int rc = mv_gemm(s, nb, L, H, F(Y.h1), H, 1, P.W2, H, 1, F(Y.ml), L, P.b2);
    if (rc) return rc;
    rc = mv_gemm(s, nb, H, L, F(Y.ml), L, 1, P.W3, L, 1, F(Y.pre2), H, P.b3);
    if (rc) return rc;
    hipLaunchKernelGGL(mv_tanh_kernel, dim3(mv_grid((long long)nb * H)), dim3(256), 0, s, (long long)nb * H, (const float *)F(Y.pre2), F(Y.h2));
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_mvae_train_epoch(const rk_mvae_desc *desc, const int32_t *user_ids, int64_t n, int32_t batch, int64_t step0, int32_t apply_update,
                                  double *losses, int32_t *status, void *stream)
{
    if (!desc || !user_ids || !losses || !status) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: a missing pointer");
    const rk_mvae_desc &D = *desc;
    rk_mvae_layout Y;
    int rc = mv_open("rk_mvae_train_epoch", D, &Y);
    if (rc) return rc;
    if (!D.m || !D.v) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: the descriptor has no Adam moments");
    if (!apply_update && !D.grad) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: apply_update = 0 needs desc.grad");
    if (batch < 1 || batch > D.ws_batch) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: batch = %d, the workspace was laid out for 1..%d", batch, D.ws_batch);
    if (n < 1 || n >= (1LL << 31)) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: n = %lld, expected 1..2^31 - 1", (long long)n);
    if (step0 < 0 || step0 + (n + batch - 1) / batch >= (1LL << 31)) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: step0 = %lld", (long long)step0);
    if (!(D.dropout >= 0.f) || !(D.dropout < 1.f)) RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: dropout must be in [0, 1)");
    if (!(D.anneal_cap >= 0.f) || !std::isfinite(D.anneal_cap) || D.total_anneal_steps < 0)
        RK_FAIL(RK_EINVAL, "rk_mvae_train_epoch: anneal_cap must be finite and >= 0, total_anneal_steps >= 0");
    hipStream_t s = (hipStream_t)stream;
    const int I = D.n_items, H = D.hidden, L = D.latent, n_steps = (int)((n + batch - 1) / batch);
    std::vector<unsigned long long> step_nnz;
    rc = mv_check_ids("rk_mvae_train_epoch", D, user_ids, n, 1, batch, n_steps, nullptr, status, &step_nnz, s);   // nothing else is launched on a bad id
    if (rc) return rc;

    char *ws = static_cast<char *>(D.workspace);
    auto F = [ws](int64_t o) { return reinterpret_cast<float *>(ws + o); };
    auto Dd = [ws](int64_t o) { return reinterpret_cast<double *>(ws + o); };
    auto Ii = [ws](int64_t o) { return reinterpret_cast<int *>(ws + o); };
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + Y.keys), *keys_in = reinterpret_cast<unsigned long long *>(ws + Y.keys_in);
    const MvPtr P(D.params, Y), G(F(Y.grad), Y);
    const double keep = 1.0 - (double)D.dropout;
    const unsigned thresh24 = (unsigned)((1.0 - (1.0 - keep)) * 16777216.0);
    const int sort_bits = mv_sort_bits(I);
    const float w1 = (float)(1.0 - (double)D.beta1), w2 = (float)(1.0 - (double)D.beta2);
    const size_t row_lds = sizeof(unsigned) * (size_t)((I + 31) / 32);
    const int hy = (H + 255) / 256;

    // the sort's scratch: stream-ordered, sized for the longest step, handed back when the call returns
    RkScratch scratch(s);
    void *sort_tmp = nullptr;
    size_t sort_cap = 0;
    const int nnz_max = (int)*std::max_element(step_nnz.begin(), step_nnz.end());
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_cap, (const unsigned long long *)keys_in, keys, nnz_max, 0, sort_bits, s));
    RK_HIP(scratch.bytes(&sort_tmp, std::max<size_t>(sort_cap, 16)));

    for (int st = 0; st < n_steps; ++st) {
        const long long first = (long long)st * batch, step = step0 + st;
        const int nb = (int)std::min<long long>(batch, n - first), nnz = (int)step_nnz[st];
        const int32_t *ids = user_ids + first;
        const double beta = D.total_anneal_steps > 0 ? std::min((double)D.anneal_cap, (double)step / (double)D.total_anneal_steps) : (double)D.anneal_cap;
        // 1: lengths, c, masks and the item-grouped view
        hipLaunchKernelGGL(mv_prep_kernel, dim3(1), dim3(256), 0, s, ids, nb, D.rowptr, keep, Ii(Y.brp), F(Y.c));
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(mv_mask_kernel, dim3(nb), dim3(256), 0, s, ids, D.rowptr, D.col, (const int *)Ii(Y.brp), I,
                           rk_drop_step_seed(D.seed, (unsigned long long)step), thresh24, Ii(Y.keep), keys_in);
        RK_CHECK_LAUNCH();
        size_t sort_bytes = sort_cap;
        RK_HIP(hipcub::DeviceRadixSort::SortKeys(sort_tmp, sort_bytes, (const unsigned long long *)keys_in, keys, nnz, 0, sort_bits, s));
        hipLaunchKernelGGL(mv_tptr_kernel, dim3((I + 1 + 255) / 256), dim3(256), 0, s, I, nnz, (const unsigned long long *)keys, Ii(Y.t_ptr));
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(mv_trow_kernel, dim3(mv_grid(nnz)), dim3(256), 0, s, nnz, (const unsigned long long *)keys, Ii(Y.t_row));
        RK_CHECK_LAUNCH();
        // 2-5: forward
        hipLaunchKernelGGL(mv_sparse_kernel, dim3(nb, hy), dim3(256), 0, s, ids, D.rowptr, D.col, (const int *)Ii(Y.brp), (const int *)Ii(Y.keep),
                           (const float *)F(Y.c), (const float *)P.W1, (const float *)P.b1, H, F(Y.a), F(Y.pre1), F(Y.h1));
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, 2 * L, H, F(Y.h1), H, 1, P.W2, H, 1, F(Y.ml), 2 * L, P.b2))) return rc;
        hipLaunchKernelGGL(mv_sample_kernel, dim3((nb + 3) / 4), dim3(256), 0, s, ids, nb, L, (const float *)F(Y.ml),
                           rk_drop_step_seed(D.seed ^ kMvEpsStream, (unsigned long long)step), F(Y.eps), F(Y.z), Dd(Y.kl));
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, H, L, F(Y.z), L, 1, P.W3, L, 1, F(Y.pre2), H, P.b3))) return rc;
        hipLaunchKernelGGL(mv_tanh_kernel, dim3(mv_grid((long long)nb * H)), dim3(256), 0, s, (long long)nb * H, (const float *)F(Y.pre2), F(Y.h2));
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, I, H, F(Y.h2), H, 1, P.W4, H, 1, F(Y.logits), I, P.b4))) return rc;
        if (D.logits_out && st == n_steps - 1)
            RK_HIP(hipMemcpyAsync(D.logits_out, F(Y.logits), sizeof(float) * (size_t)nb * I, hipMemcpyDeviceToDevice, s));
        // 6: loss and dl, in place
        hipLaunchKernelGGL(mv_row_kernel, dim3(nb), dim3(256), row_lds, s, ids, D.rowptr, D.col, I, nb, F(Y.logits), Dd(Y.lse), Dd(Y.nll));
        RK_CHECK_LAUNCH();
        // 7: backward
        const float *dl = F(Y.logits);
        if ((rc = mv_gemm(s, I, H, nb, dl, 1, I, F(Y.h2), 1, H, G.W4, H, nullptr))) return rc;
        hipLaunchKernelGGL(mv_colsum_kernel, dim3((I + 255) / 256), dim3(256), 0, s, nb, I, dl, G.b4);
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, H, I, dl, I, 1, P.W4, 1, H, F(Y.dh2), H, nullptr))) return rc;
        hipLaunchKernelGGL(mv_tanh_bwd_kernel, dim3(mv_grid((long long)nb * H)), dim3(256), 0, s, (long long)nb * H, (const float *)F(Y.dh2),
                           (const float *)F(Y.h2), F(Y.dp2));
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, H, L, nb, F(Y.dp2), 1, H, F(Y.z), 1, L, G.W3, L, nullptr))) return rc;
        hipLaunchKernelGGL(mv_colsum_kernel, dim3((H + 255) / 256), dim3(256), 0, s, nb, H, (const float *)F(Y.dp2), G.b3);
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, L, H, F(Y.dp2), H, 1, P.W3, 1, L, F(Y.dz), L, nullptr))) return rc;
        hipLaunchKernelGGL(mv_sample_bwd_kernel, dim3(mv_grid((long long)nb * L)), dim3(256), 0, s, nb, L, (const float *)F(Y.dz), (const float *)F(Y.ml),
                           (const float *)F(Y.eps), beta / (double)nb, beta / (2.0 * (double)nb), F(Y.dml));
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, 2 * L, H, nb, F(Y.dml), 1, 2 * L, F(Y.h1), 1, H, G.W2, H, nullptr))) return rc;
        hipLaunchKernelGGL(mv_colsum_kernel, dim3((2 * L + 255) / 256), dim3(256), 0, s, nb, 2 * L, (const float *)F(Y.dml), G.b2);
        RK_CHECK_LAUNCH();
        if ((rc = mv_gemm(s, nb, H, 2 * L, F(Y.dml), 2 * L, 1, P.W2, 1, H, F(Y.dh1), H, nullptr))) return rc;
        hipLaunchKernelGGL(mv_tanh_bwd_kernel, dim3(mv_grid((long long)nb * H)), dim3(256), 0, s, (long long)nb * H, (const float *)F(Y.dh1),
                           (const float *)F(Y.h1), F(Y.dp1));
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(mv_gw1_kernel, dim3(I, hy), dim3(256), 0, s, (const int *)Ii(Y.t_ptr), (const int *)Ii(Y.t_row), (const float *)F(Y.c),
                           (const float *)F(Y.dp1), H, G.W1);
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(mv_colsum_kernel, dim3((H + 255) / 256), dim3(256), 0, s, nb, H, (const float *)F(Y.dp1), G.b1);
        RK_CHECK_LAUNCH();
        // 8: Adam and the step's losses
        const AdamCoef co = adam_coef((int)(step + 1), D.lr, D.beta1, D.beta2);
        hipLaunchKernelGGL(mv_adam_kernel, dim3(mv_grid(Y.n_params)), dim3(256), 0, s, (long long)Y.n_params, D.params, (const float *)F(Y.grad), D.m, D.v,
                           apply_update ? (float *)nullptr : D.grad, apply_update, co.step_size, co.bc2s, D.beta2, w1, w2, D.adam_eps,
                           (const double *)Dd(Y.nll), (const double *)Dd(Y.kl), nb, beta, losses + 3 * (size_t)st);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}

RK_EXPORT int rk_mvae_scores(const rk_mvae_desc *desc, const int32_t *user_ids, int32_t nb, float *out, int64_t ldo, void *stream)
{
    if (!desc || !user_ids || !out) RK_FAIL(RK_EINVAL, "rk_mvae_scores: a missing pointer");
    const rk_mvae_desc &D = *desc;
    rk_mvae_layout Y;
    int rc = mv_open("rk_mvae_scores", D, &Y);
    if (rc) return rc;
    if (nb < 1) RK_FAIL(RK_EINVAL, "rk_mvae_scores: nb = %d", nb);
    if (ldo < D.n_items || ldo >= (1LL << 31)) RK_FAIL(RK_EINVAL, "rk_mvae_scores: ldo = %lld, expected n_items..2^31 - 1", (long long)ldo);
    hipStream_t s = (hipStream_t)stream;
    rc = mv_check_ids("rk_mvae_scores", D, user_ids, nb, 0, 1, 1, nullptr, nullptr, nullptr, s);
    if (rc) return rc;
    const MvPtr P(D.params, Y);
    float *h2 = reinterpret_cast<float *>(static_cast<char *>(D.workspace) + Y.h2);
    for (int r0 = 0; r0 < nb; r0 += D.ws_batch) {
        const int rows = std::min(D.ws_batch, nb - r0);
        if ((rc = mv_infer_h2(D, Y, user_ids + r0, rows, s))) return rc;
        if ((rc = mv_gemm(s, rows, D.n_items, D.hidden, h2, D.hidden, 1, P.W4, D.hidden, 1, out + (size_t)r0 * ldo, (int)ldo, P.b4))) return rc;
    }
    return RK_OK;
}

RK_EXPORT int rk_mvae_pair_scores(const rk_mvae_desc *desc, const int32_t *user_ids, const int32_t *item_ids, int64_t n, float *out, void *stream)
{
    if (!desc) RK_FAIL(RK_EINVAL, "rk_mvae_pair_scores: a missing pointer");
    if (n == 0) return RK_OK;
    if (!user_ids || !item_ids || !out) RK_FAIL(RK_EINVAL, "rk_mvae_pair_scores: a missing pointer");
    const rk_mvae_desc &D = *desc;
    rk_mvae_layout Y;
    int rc = mv_open("rk_mvae_pair_scores", D, &Y);
    if (rc) return rc;
    if (n < 0 || n >= (1LL << 31)) RK_FAIL(RK_EINVAL, "rk_mvae_pair_scores: n = %lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    rc = mv_check_ids("rk_mvae_pair_scores", D, user_ids, n, 0, 1, 1, item_ids, nullptr, nullptr, s);
    if (rc) return rc;
    const MvPtr P(D.params, Y);
    const float *h2 = reinterpret_cast<const float *>(static_cast<char *>(D.workspace) + Y.h2);
    for (int64_t r0 = 0; r0 < n; r0 += D.ws_batch) {
        const int rows = (int)std::min<int64_t>(D.ws_batch, n - r0);
        if ((rc = mv_infer_h2(D, Y, user_ids + r0, rows, s))) return rc;
        hipLaunchKernelGGL(mv_pair_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, rows, D.hidden, h2, item_ids + r0, (const float *)P.W4,
                           (const float *)P.b4, out + r0);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}
