// AushPlus attacker (recad/model/attacker/aushplus.py) on the device: the discretising autoencoder generator, its projection
// with the tanh surrogate gradient of the Heaviside, and the discriminator.  The surrogate fits of its attack phase are
// aia.hip's; the Adam steps are rk_adam_step over the packed parameter arrays.
//
// Every consumer reads the generator only where the input row is non-zero, so everything here works on a CSR of rows:
//   * G forward, one workgroup (128 threads = the hidden units, 125 padded to 128) per row: the first layer is a gather-sum of
//     the item-major W1^T rows of the row's non-zeros, the second layer a SAMPLED product (a[r, j] for j in nnz(r) only, one
//     wave per entry), then tanh, the boundaries and the class / value per stored entry.  Nothing rows x I is formed.
//   * G backward: per row, the surrogate gradient into z-bar (pre-tanh) and the four boundary gradients per entry, then
//     h1-bar through the sampled W2 rows and the relu; per ITEM, the rows of W2 / W1^T / b2 / min_boundary / interval_lengths
//     summed over the item's entries through a transposed entry list in a fixed order; b1 over the rows in row order.
//   * D: one workgroup (512 threads) per row does the sparse first layer, 512 -> 128 -> 1 as plain VALU dot products (at most
//     2 x attack_num rows: too small for the matrix cores to matter), the BCE, and the whole backward down to dL/d(input value)
//     at the row's entries; the weight gradients are reduced per unit / per item over the rows in row order.
// No float atomics: every reduction has a fixed order, so two runs give the same bits.  Item rows no entry touches get an
// exact 0 gradient, which leaves them where they are under Adam as long as they never saw another one.
#include "common.h"

namespace {

constexpr int HG = RK_AP_HG;      // 128
constexpr int H1 = RK_AP_HD1;     // 512
constexpr int H2 = RK_AP_HD2;     // 128

struct GParams {
    const float *w1t, *b1, *w2, *b2, *minb, *ilen;
};

__host__ __device__ inline GParams g_params(const float *p, int I)
{
    GParams g;
    g.w1t = p;
    g.b1 = g.w1t + (size_t)I * HG;
    g.w2 = g.b1 + HG;
    g.b2 = g.w2 + (size_t)I * HG;
    g.minb = g.b2 + I;
    g.ilen = g.minb + I;
    return g;
}

// get_boundary_values (aushplus.py:370-378): b0 = min_boundary, b_k = b_{k-1} + (relu(len_{k-1}) + 1e-4), each rounded on its own
__device__ __forceinline__ void boundaries(const float *__restrict__ minb, const float *__restrict__ ilen, int j, float b[4])
{
#pragma clang fp contract(off)
    b[0] = minb[j];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float cur = fmaxf(ilen[3 * (size_t)j + k - 1], 0.f) + 1e-4f;
        b[k] = b[k - 1] + cur;
    }
}

// H_ck = [s_ck (a - b_k) > 0], s_ck = sign(c - k - 0.5): +1 for k < c, -1 otherwise
__device__ __forceinline__ bool hv(int c, int k, float d) { return k < c ? d > 0.f : -d > 0.f; }

__device__ __forceinline__ float act_a(float z)
{
#pragma clang fp contract(off)
    const float h = tanhf(z);
    return h * 2.5f + 2.5f;
}

// ---------------------------------------------------------------- generator forward
__global__ __launch_bounds__(128) void g_forward_kernel(int I, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                        const float *__restrict__ x, const float *__restrict__ gp,
                                                        float *__restrict__ norm, float *__restrict__ h1o, float *__restrict__ a_out,
                                                        int *__restrict__ cls_out, float *__restrict__ val_out)
{
    __shared__ float sh1[HG];
    const GParams g = g_params(gp, I);
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int b = rowptr[r], e = rowptr[r + 1];
    float s2 = 0.f, acc = 0.f;
    for (int k = b; k < e; ++k) {
        const float xk = x[k];
        s2 += xk * xk;
        acc += xk * g.w1t[(size_t)col[k] * HG + t];
    }
    const float nrm = fmaxf(sqrtf(s2), 1e-12f);      // F.normalize: x / max(||x||, eps)
    const float h = fmaxf(acc / nrm + g.b1[t], 0.f);
    sh1[t] = h;
    h1o[(size_t)r * HG + t] = h;
    if (t == 0) norm[r] = nrm;
    __syncthreads();
    for (int k = b + w; k < e; k += 2) {
        const int j = col[k];
        const float *wr = g.w2 + (size_t)j * HG;
        const float z = wave_sum(wr[lane] * sh1[lane] + wr[64 + lane] * sh1[64 + lane]) + g.b2[j];
        if (lane == 0) {
            const float a = act_a(z);
            float bd[4];
            boundaries(g.minb, g.ilen, j, bd);
            int cls = -1;
            float value = 0.f;
            for (int c = 0; c < 5; ++c) {
                bool on = true;
                for (int kk = 0; kk < 4; ++kk) on = on && hv(c, kk, a - bd[kk]);
                if (on) {
                    cls = c;
                    value += (float)(c + 1);
                }
            }
            a_out[k] = a;
            cls_out[k] = cls;
            val_out[k] = x[k] > 0.f ? value : 0.f;    // fake_dsct_value * (input > 0)
        }
    }
}

// ---------------------------------------------------------------- generator backward, per row
// mode 0: dL/dvalue per entry given (masked by x > 0); mode 1: CrossEntropyLoss of the five 0/1 products against x - 1 over the
// entries with x > 0, mean over n = 1 / scale of them.
__global__ __launch_bounds__(128) void g_row_backward_kernel(int I, int mode, float scale, const int *__restrict__ rowptr,
                                                             const int *__restrict__ col, const float *__restrict__ x,
                                                             const float *__restrict__ gp, const float *__restrict__ h1,
                                                             const float *__restrict__ a_in, const float *__restrict__ dvalue,
                                                             float *__restrict__ zbar, float *__restrict__ bbar,
                                                             float *__restrict__ eloss, float *__restrict__ dpre)
{
    const GParams g = g_params(gp, I);
    const int r = blockIdx.x, t = threadIdx.x;
    const int b = rowptr[r], e = rowptr[r + 1];
    for (int k = b + t; k < e; k += 128) {
        const int j = col[k];
        const float a = a_in[k], xk = x[k];
        float bd[4], d[4], gc[5];
        boundaries(g.minb, g.ilen, j, bd);
        for (int kk = 0; kk < 4; ++kk) d[kk] = a - bd[kk];
        float el = 0.f;
        if (mode == 0) {
            const float dv = xk > 0.f ? dvalue[k] : 0.f;
            for (int c = 0; c < 5; ++c) gc[c] = (float)(c + 1) * dv;
        } else {
            float dist[5], se = 0.f;
            for (int c = 0; c < 5; ++c) {
                bool on = true;
                for (int kk = 0; kk < 4; ++kk) on = on && hv(c, kk, d[kk]);
                dist[c] = on ? 1.f : 0.f;
                se += expf(dist[c]);
            }
            const float lse = logf(se);
            const int y = (int)xk - 1;
            const bool use = xk > 0.f && y >= 0 && y < 5;
            for (int c = 0; c < 5; ++c) gc[c] = use ? (expf(dist[c] - lse) - (c == y ? 1.f : 0.f)) * scale : 0.f;
            el = use ? (lse - dist[y]) * scale : 0.f;
        }
        // HeaviTanh backward through rating_prob *= H_k: d dist_c / d d_k = s_ck sech^2(d_k) prod_{l != k} H_cl
        float abar = 0.f;
        for (int kk = 0; kk < 4; ++kk) {
            const float th = tanhf(d[kk]);
            const float sech2 = 1.f - th * th;
            float dd = 0.f;
            for (int c = 0; c < 5; ++c) {
                bool others = true;
                for (int l = 0; l < 4; ++l)
                    if (l != kk) others = others && hv(c, l, d[l]);
                if (others) dd += (kk < c ? gc[c] : -gc[c]) * sech2;
            }
            abar += dd;
            bbar[4 * (size_t)k + kk] = -dd;
        }
        const float h2 = (a - 2.5f) / 2.5f;
        zbar[k] = abar * 2.5f * (1.f - h2 * h2);
        eloss[k] = el;
    }
    // zbar[b .. e) was written above by this workgroup's own threads and is read back here by all of them: the barrier orders the
    // global writes inside the workgroup, and no other pointer aliases zbar (which is what its __restrict__ says)
    __syncthreads();
    float acc = 0.f;
    for (int k = b; k < e; ++k) acc += zbar[k] * g.w2[(size_t)col[k] * HG + t];
    dpre[(size_t)r * HG + t] = h1[(size_t)r * HG + t] > 0.f ? acc : 0.f;
}

// ---------------------------------------------------------------- generator backward, per item (transposed entry list)
__global__ __launch_bounds__(128) void g_item_backward_kernel(int I, const int *__restrict__ tptr, const int *__restrict__ tent,
                                                              const int *__restrict__ trow, const float *__restrict__ x,
                                                              const float *__restrict__ gp, const float *__restrict__ norm,
                                                              const float *__restrict__ h1, const float *__restrict__ dpre,
                                                              const float *__restrict__ zbar, const float *__restrict__ bbar,
                                                              float *__restrict__ grad)
{
    const GParams g = g_params(gp, I);
    const int j = blockIdx.x, t = threadIdx.x;
    float gw1 = 0.f, gw2 = 0.f, side = 0.f;
    for (int q = tptr[j]; q < tptr[j + 1]; ++q) {
        const int k = tent[q], r = trow[q];
        const float zb = zbar[k];
        gw2 += zb * h1[(size_t)r * HG + t];
        gw1 += (x[k] / norm[r]) * dpre[(size_t)r * HG + t];
        if (t == 0) side += zb;                                   // b2
        else if (t == 1) side += bbar[4 * (size_t)k] + bbar[4 * (size_t)k + 1] + bbar[4 * (size_t)k + 2] + bbar[4 * (size_t)k + 3];
        else if (t == 2) side += bbar[4 * (size_t)k + 1] + bbar[4 * (size_t)k + 2] + bbar[4 * (size_t)k + 3];
        else if (t == 3) side += bbar[4 * (size_t)k + 2] + bbar[4 * (size_t)k + 3];
        else if (t == 4) side += bbar[4 * (size_t)k + 3];
    }
    float *gw1t = grad, *gb2 = grad + (size_t)I * HG + HG + (size_t)I * HG, *gminb = gb2 + I, *gilen = gminb + I;
    gw1t[(size_t)j * HG + t] = gw1;
    (grad + (size_t)I * HG + HG)[(size_t)j * HG + t] = gw2;
    if (t == 0) gb2[j] = side;
    else if (t == 1) gminb[j] = side;
    else if (t <= 4) gilen[3 * (size_t)j + t - 2] = g.ilen[3 * (size_t)j + t - 2] > 0.f ? side : 0.f;    // relu'
}

// column sums in row order: out[t] = sum_r in[r * width + t]
__global__ void colsum_kernel(int n_rows, int width, const float *__restrict__ in, float *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= width) return;
    float s = 0.f;
    for (int r = 0; r < n_rows; ++r) s += in[(size_t)r * width + t];
    out[t] = s;
}

// out[0] = sum of in[0 .. n) in a fixed order (256 strided partials, then a fixed tree)
__global__ __launch_bounds__(256) void sum_kernel(long long n, const float *__restrict__ in, float *__restrict__ out)
{
    __shared__ float red[256];
    float s = 0.f;
    for (long long k = threadIdx.x; k < n; k += 256) s += in[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---------------------------------------------------------------- discriminator
struct DArgs {
    int I, nA, nB;
    const int *rowptrA, *colA, *rowptrB, *colB;
    const float *valA, *valB;
    float labelA, labelB;
    const float *dp;
    float *work, *dinB;
};

struct DWork {
    float *h1, *dz1, *h2, *dz2, *p, *dlogit, *rowloss;
};
__host__ __device__ inline DWork d_work(float *w, int n)
{
    DWork o;
    o.h1 = w;
    o.dz1 = o.h1 + (size_t)n * H1;
    o.h2 = o.dz1 + (size_t)n * H1;
    o.dz2 = o.h2 + (size_t)n * H2;
    o.p = o.dz2 + (size_t)n * H2;
    o.dlogit = o.p + n;
    o.rowloss = o.dlogit + n;
    return o;
}

__global__ __launch_bounds__(512) void d_row_kernel(DArgs a)
{
    __shared__ float sh1[H1];
    __shared__ float sh2[H2];
    __shared__ float sdz2[H2];
    __shared__ float sdl;
    const int n = a.nA + a.nB, r = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const bool isA = r < a.nA;
    const int *rowptr = isA ? a.rowptrA : a.rowptrB, *col = isA ? a.colA : a.colB;
    const float *val = isA ? a.valA : a.valB;
    const int lr = isA ? r : r - a.nA;
    const int b = rowptr[lr], e = rowptr[lr + 1];
    const float y = isA ? a.labelA : a.labelB, wgt = 1.f / (float)(isA ? a.nA : a.nB);
    const float *w1t = a.dp, *b1 = w1t + (size_t)a.I * H1, *W2 = b1 + H1, *b2 = W2 + (size_t)H2 * H1, *w3 = b2 + H2, *b3 = w3 + H2;
    const DWork wk = d_work(a.work, n);
    float acc = 0.f;
    for (int k = b; k < e; ++k) acc += val[k] * w1t[(size_t)col[k] * H1 + t];
    const float h1 = fmaxf(acc + b1[t], 0.f);
    sh1[t] = h1;
    wk.h1[(size_t)r * H1 + t] = h1;
    __syncthreads();
    for (int u = w * 16; u < w * 16 + 16; ++u) {
        const float *wr = W2 + (size_t)u * H1;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < H1 / 64; ++i) s += wr[lane + 64 * i] * sh1[lane + 64 * i];
        s = wave_sum(s);
        if (lane == 0) sh2[u] = fmaxf(s + b2[u], 0.f);
    }
    __syncthreads();
    if (w == 0) {
        const float s = wave_sum(w3[lane] * sh2[lane] + w3[lane + 64] * sh2[lane + 64]) + b3[0];
        if (lane == 0) {
            const float p = 1.f / (1.f + expf(-s));
            // nn.BCELoss: the logs are clamped at -100; its backward divides by max((1 - p) p, 1e-12), the sigmoid's multiplies back
            const float l = -(y * fmaxf(logf(p), -100.f) + (1.f - y) * fmaxf(logf(1.f - p), -100.f));
            const float dl = (p - y) / fmaxf((1.f - p) * p, 1e-12f) * (p * (1.f - p)) * wgt;
            wk.p[r] = p;
            wk.rowloss[r] = l * wgt;
            wk.dlogit[r] = dl;
            sdl = dl;
        }
    }
    __syncthreads();
    if (t < H2) {
        const float h2 = sh2[t];
        const float dz = h2 > 0.f ? sdl * w3[t] : 0.f;
        sdz2[t] = dz;
        wk.h2[(size_t)r * H2 + t] = h2;
        wk.dz2[(size_t)r * H2 + t] = dz;
    }
    __syncthreads();
    float dh = 0.f;
    for (int u = 0; u < H2; ++u) dh += sdz2[u] * W2[(size_t)u * H1 + t];
    const float dz1 = h1 > 0.f ? dh : 0.f;
    wk.dz1[(size_t)r * H1 + t] = dz1;
    if (isA || !a.dinB) return;
    __syncthreads();          // sh1 is reused for dz1 (every thread of the workgroup takes this path together)
    sh1[t] = dz1;
    __syncthreads();
    for (int k = b + w; k < e; k += 8) {
        const float *wr = w1t + (size_t)col[k] * H1;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < H1 / 64; ++i) s += wr[lane + 64 * i] * sh1[lane + 64 * i];
        s = wave_sum(s);
        if (lane == 0) a.dinB[k] = s;
    }
}

// blocks 0 .. 127: row u of W2-bar and b2-bar[u]; block 128: b1-bar, w3-bar, b3-bar.  Sums over the rows in row order.
__global__ __launch_bounds__(512) void d_dense_grad_kernel(int I, int n, const float *__restrict__ work_c, float *__restrict__ grad)
{
    const DWork wk = d_work(const_cast<float *>(work_c), n);
    float *gb1 = grad + (size_t)I * H1, *gW2 = gb1 + H1, *gb2 = gW2 + (size_t)H2 * H1, *gw3 = gb2 + H2, *gb3 = gw3 + H2;
    const int t = threadIdx.x, u = blockIdx.x;
    if (u < H2) {
        float s = 0.f, sb = 0.f;
        for (int r = 0; r < n; ++r) {
            const float dz = wk.dz2[(size_t)r * H2 + u];
            s += dz * wk.h1[(size_t)r * H1 + t];
            sb += dz;
        }
        gW2[(size_t)u * H1 + t] = s;
        if (t == 0) gb2[u] = sb;
        return;
    }
    float s = 0.f, s3 = 0.f, sb = 0.f;
    for (int r = 0; r < n; ++r) {
        s += wk.dz1[(size_t)r * H1 + t];
        if (t < H2) s3 += wk.dlogit[r] * wk.h2[(size_t)r * H2 + t];
        if (t == 0) sb += wk.dlogit[r];
    }
    gb1[t] = s;
    if (t < H2) gw3[t] = s3;
    if (t == 0) gb3[0] = sb;
}

// W1^T-bar row of item j: sum over the item's entries, in list order, of value * dz1[row]
__global__ __launch_bounds__(512) void d_item_grad_kernel(int nA, int n, const int *__restrict__ tptr, const int *__restrict__ trow,
                                                          const int *__restrict__ tsrc, const float *__restrict__ valA,
                                                          const float *__restrict__ valB, const float *__restrict__ work_c,
                                                          float *__restrict__ grad)
{
    const DWork wk = d_work(const_cast<float *>(work_c), n);
    const int j = blockIdx.x, t = threadIdx.x;
    float s = 0.f;
    for (int q = tptr[j]; q < tptr[j + 1]; ++q) {
        const int r = trow[q];
        const float v = r < nA ? valA[tsrc[q]] : valB[tsrc[q]];
        s += v * wk.dz1[(size_t)r * H1 + t];
    }
    grad[(size_t)j * H1 + t] = s;
}

}  // namespace

RK_EXPORT int rk_ap_g_forward(int32_t n_rows, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *x, const float *gparam,
                              float *norm, float *h1, float *a, int32_t *cls, float *value, void *stream)
{
    if (n_rows < 0 || n_items <= 0 || (n_rows > 0 && (!rowptr || !col || !x || !gparam || !norm || !h1 || !a || !cls || !value)))
        RK_FAIL(RK_EINVAL, "rk_ap_g_forward: bad arguments");
    if (n_rows == 0) return RK_OK;
    hipLaunchKernelGGL(g_forward_kernel, dim3(n_rows), dim3(128), 0, (hipStream_t)stream, n_items, rowptr, col, x, gparam, norm, h1, a, cls,
                       value);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_ap_g_backward(int32_t n_rows, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *x,
                               const float *gparam, const float *norm, const float *h1, const float *a, int32_t mode, const float *dvalue,
                               float scale, int64_t entry0, int64_t n_entries, const int32_t *tptr, const int32_t *tent, const int32_t *trow, float *zbar,
                               float *bbar, float *eloss, float *dpre, float *ggrad, float *loss, void *stream)
{
    if (n_rows <= 0 || n_items <= 0 || entry0 < 0 || n_entries < 0 || !rowptr || !col || !x || !gparam || !norm || !h1 || !a || (mode != 0 && mode != 1) ||
        (mode == 0 && !dvalue) || !tptr || !tent || !trow || !zbar || !bbar || !eloss || !dpre || !ggrad || (mode == 1 && !loss))
        RK_FAIL(RK_EINVAL, "rk_ap_g_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(g_row_backward_kernel, dim3(n_rows), dim3(128), 0, s, n_items, mode, scale, rowptr, col, x, gparam, h1, a, dvalue, zbar,
                       bbar, eloss, dpre);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(g_item_backward_kernel, dim3(n_items), dim3(128), 0, s, n_items, tptr, tent, trow, x, gparam, norm, h1, dpre, zbar, bbar,
                       ggrad);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_kernel, dim3(1), dim3(HG), 0, s, n_rows, HG, dpre, ggrad + (size_t)n_items * HG);
    RK_CHECK_LAUNCH();
    if (mode == 1) {
        hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (long long)n_entries, eloss + entry0, loss);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}

RK_EXPORT int rk_ap_d_step(int32_t n_items, int32_t nA, const int32_t *rowptrA, const int32_t *colA, const float *valA, float labelA,
                           int32_t nB, const int32_t *rowptrB, const int32_t *colB, const float *valB, float labelB, const float *dparam,
                           float *work, const int32_t *tptr, const int32_t *trow, const int32_t *tsrc, float *dgrad, float *dinB,
                           float *loss, void *stream)
{
    const int n = nA + nB;
    if (n_items <= 0 || nA < 0 || nB < 0 || n <= 0 || (nA > 0 && (!rowptrA || !colA || !valA)) || (nB > 0 && (!rowptrB || !colB || !valB)) ||
        !dparam || !work || !loss || (dgrad && (!tptr || !trow || !tsrc)))
        RK_FAIL(RK_EINVAL, "rk_ap_d_step: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    DArgs a{};
    a.I = n_items;
    a.nA = nA;
    a.nB = nB;
    a.rowptrA = rowptrA;
    a.colA = colA;
    a.valA = valA;
    a.rowptrB = rowptrB;
    a.colB = colB;
    a.valB = valB;
    a.labelA = labelA;
    a.labelB = labelB;
    a.dp = dparam;
    a.work = work;
    a.dinB = dinB;
    hipLaunchKernelGGL(d_row_kernel, dim3(n), dim3(512), 0, s, a);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, s, (long long)n, d_work(work, n).rowloss, loss);
    RK_CHECK_LAUNCH();
    if (dgrad) {
        hipLaunchKernelGGL(d_dense_grad_kernel, dim3(H2 + 1), dim3(512), 0, s, n_items, n, work, dgrad);
        RK_CHECK_LAUNCH();
        hipLaunchKernelGGL(d_item_grad_kernel, dim3(n_items), dim3(512), 0, s, nA, n, tptr, trow, tsrc, valA, valB, work, dgrad);
        RK_CHECK_LAUNCH();
    }
    return RK_OK;
}
