// AUSH attacker (recad/model/attacker/aush.py) on the device.  The reference slices dense B x I rows out of the
// dense U x I train_mat (explicit.py:102,178-199) and runs dense generator / discriminator GEMMs over them; here
// nothing U x I or B x I is formed.  Every row of the attack is the sparse set "fillers U S" (<= filler_num + |S|
// entries), so
//   * the eligible users and the filler pool come from the rating CSR (rk_aush_eligible),
//   * the generator is evaluated at S only (rk_aush_gen; the reference never trains it, aush.py:138),
//   * the discriminator's first layer gathers <= filler_num + |S| rows of its item-major weight, and its gradient
//     is a scatter onto those rows, reduced in (item, row) order after a radix sort: no float atomics, so two runs
//     with the same seed are bit-identical (rk_aush_d_step),
//   * Adam runs over the dense tail of D and over the first-layer rows touched so far (rk_aush_d_step).
// Random draws come from rk_mix64, keyed on (seed, stream, row, draw): the stream is the epoch for training and a
// per-call id for generate_fake.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int HG = RK_AUSH_HG;
constexpr int HD = RK_AUSH_HD;
constexpr int kSentinel = 0x7fffffff;

__device__ __forceinline__ float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

__device__ __forceinline__ bool in_sorted(const int *__restrict__ a, int n, int c) { return rk_find_sorted(a, 0, n, c) >= 0; }

// ---------------------------------------------------------------- eligible users and filler pool
// pool_cnt[u] = #{rated items of u (value > 0) outside excl} -- the set the reference draws fillers from
// (aush.py:63-70) and counts for eligibility (utils.py:192-196, aush.py:177-180).
__global__ void pool_count_kernel(int n_users, const int *__restrict__ rowptr, const int *__restrict__ col,
                                  const float *__restrict__ val, const int *__restrict__ excl, int n_excl, int *__restrict__ cnt)
{
    const int u = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= n_users) return;
    int c = 0;
    for (int k = rowptr[u] + lane; k < rowptr[u + 1]; k += 64)
        c += (val[k] > 0.f && !in_sorted(excl, n_excl, col[k])) ? 1 : 0;
    c = wave_sum(c);
    if (lane == 0) cnt[u] = c;
}

// one wave per user: the pool entries in row order (ascending item), by a wave-wide prefix count
__global__ void pool_fill_kernel(int n_users, const int *__restrict__ rowptr, const int *__restrict__ col,
                                 const float *__restrict__ val, const int *__restrict__ excl, int n_excl,
                                 const int *__restrict__ pool_ptr, int *__restrict__ pool_col, int filler_num,
                                 int *__restrict__ flag)
{
    const int u = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (u >= n_users) return;
    int out = pool_ptr[u];
    for (int k0 = rowptr[u]; k0 < rowptr[u + 1]; k0 += 64) {
        const int k = k0 + lane;
        const bool keep = k < rowptr[u + 1] && val[k] > 0.f && !in_sorted(excl, n_excl, col[k]);
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (keep) pool_col[out + before] = col[k];
        out += __popcll(bal);
    }
    if (lane == 0) flag[u] = (pool_ptr[u + 1] - pool_ptr[u]) >= filler_num ? 1 : 0;
}

// ---------------------------------------------------------------- permutation
__global__ void perm_keys_kernel(int n, unsigned long long seed, unsigned long long stream, unsigned long long *__restrict__ keys,
                                 int *__restrict__ pos)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = rk_draw_key(seed, stream, i, 0x7ffff);
    pos[i] = i;
}

__global__ void gather_kernel(int n, const int *__restrict__ src, const int *__restrict__ pos, int *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[pos[i]];
}

// ---------------------------------------------------------------- filler draws
// One wave per row.  draws[r, d] (given) or the RNG's pool pick; duplicates collapse (the reference's 0/1
// fillers_mask, aush.py:74-75); the distinct fillers are written ascending with their ratings; sval = rating at S.
__global__ __launch_bounds__(64) void sample_kernel(int n_rows, const int *__restrict__ users, int F, const int *__restrict__ rowptr,
                                                    const int *__restrict__ col, const float *__restrict__ val,
                                                    const int *__restrict__ pool_ptr, const int *__restrict__ pool_col,
                                                    const int *__restrict__ draws, unsigned long long seed, unsigned long long stream,
                                                    long long row0, const int *__restrict__ sel, int n_sel, int *__restrict__ fcol,
                                                    float *__restrict__ fval, int *__restrict__ nf, float *__restrict__ sval)
{
    __shared__ int d[RK_AUSH_MAX_FILLER];
    __shared__ int keep[RK_AUSH_MAX_FILLER];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= n_rows) return;
    const int u = users[r];
    const int rb = rowptr[u], re = rowptr[u + 1];
    for (int k = lane; k < F; k += 64) {
        int c;
        if (draws) {
            c = draws[(long long)r * F + k];
        } else {
            const int pb = pool_ptr[u], deg = pool_ptr[u + 1] - pb;
            const unsigned long long x = rk_draw_key(seed, stream, row0 + r, k);
            c = deg > 0 ? pool_col[pb + (int)(((x >> 32) * (unsigned long long)deg) >> 32)] : kSentinel;
        }
        d[k] = c;
    }
    __syncthreads();
    for (int k = lane; k < F; k += 64) {
        bool first = d[k] != kSentinel;
        for (int j = 0; j < k && first; ++j) first = d[j] != d[k];
        keep[k] = first ? 1 : 0;
    }
    __syncthreads();
    int n_keep = 0;
    for (int k = 0; k < F; ++k) n_keep += keep[k];
    for (int k = lane; k < F; k += 64) {
        const long long o = (long long)r * F;
        if (keep[k]) {
            int rank = 0;
            for (int j = 0; j < F; ++j) rank += (keep[j] && d[j] < d[k]) ? 1 : 0;
            const int p = rk_find_sorted(col, rb, re, d[k]);
            fcol[o + rank] = d[k];
            fval[o + rank] = p >= 0 ? val[p] : 0.f;
        }
        if (k >= n_keep) { fcol[o + k] = kSentinel; fval[o + k] = 0.f; }
    }
    for (int s = lane; s < n_sel; s += 64) {
        const int p = rk_find_sorted(col, rb, re, sel[s]);
        sval[(long long)r * n_sel + s] = p >= 0 ? val[p] : 0.f;
    }
    if (lane == 0) nf[r] = n_keep;
}

// ---------------------------------------------------------------- ZR mask (aush.py:114-119)
// One block per batch: of the (row, s) pairs whose real rating is 0, keep the n - floor(n * (1 - ZR_ratio)) of
// smallest random key (a uniform subset of exactly that size; the reference shuffles and zeroes a prefix).
__global__ __launch_bounds__(1024) void zr_kernel(int n_rows, int batch, int n_sel, const float *__restrict__ sval, double zr_ratio,
                                                  unsigned long long seed, unsigned long long stream, unsigned char *__restrict__ zr)
{
    __shared__ unsigned long long key[RK_AUSH_MAX_PAIRS];
    __shared__ int cnt;
    const int r0 = blockIdx.x * batch, rows = min(batch, n_rows - r0), P = rows * n_sel;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const bool z = sval[(long long)r0 * n_sel + p] == 0.f;
        key[p] = z ? (rk_draw_key(seed, stream ^ 0x5a5a5a5aULL, r0 + p / n_sel, 0x40000 + p % n_sel) | 1ULL) : 0ULL;
        if (z) atomicAdd(&cnt, 1);
    }
    __syncthreads();
    const int n = cnt;
    const int n_keep = n - (int)floor((double)n * (1.0 - zr_ratio));
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
        const unsigned long long k = key[p];
        int rank = 0;
        if (k) {
            for (int q = 0; q < P; ++q) {
                const unsigned long long kq = key[q];
                rank += (kq && (kq < k || (kq == k && q < p))) ? 1 : 0;
            }
        }
        zr[(long long)r0 * n_sel + p] = (k && rank < n_keep) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- generator at S (aush.py:211-222)
// gen[r, s] = 5 sigma(W2[sel_s] . sigma(W1 template_r + b1) + b2[sel_s]); the template is the row's fillers.
__global__ __launch_bounds__(HG) void gen_kernel(int n_rows, int F, const int *__restrict__ fcol, const float *__restrict__ fval,
                                                 const int *__restrict__ nf, const float *__restrict__ w1t, const float *__restrict__ b1,
                                                 const float *__restrict__ w2, const float *__restrict__ b2, const int *__restrict__ sel,
                                                 int n_sel, float *__restrict__ gen)
{
    __shared__ float h[HG];
    __shared__ float part[HG / 64];
    const int r = blockIdx.x, j = threadIdx.x;
    if (r >= n_rows) return;
    const int n = nf[r];
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc += fval[(long long)r * F + k] * w1t[(long long)fcol[(long long)r * F + k] * HG + j];
    h[j] = sigm(acc + b1[j]);
    __syncthreads();
    for (int s = 0; s < n_sel; ++s) {
        const float v = wave_sum(w2[(long long)sel[s] * HG + j] * h[j]);
        if ((j & 63) == 0) part[j >> 6] = v;
        __syncthreads();
        if (j == 0) gen[(long long)r * n_sel + s] = sigm(part[0] + part[1] + b2[sel[s]]) * 5.0f;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- discriminator (aush.py:225-241)
struct DWork {
    int B, F, n_sel, E;   // E = B * (F + n_sel) entries (padding included)
    float *h1, *h2, *h3, *dz1, *dz2, *dz3, *dz4, *bce;   // rows: [0, B) real, [B, 2B) fake; bce [3B]: real, fake, gan
    float *gtail, *gbuf;
    int *ecol;
    float *eval_r, *eval_f;
    unsigned long long *keys, *keys_sorted;
    int *flag, *segid, *seg_start, *ucol, *counts;   // counts: [0] n_unique, [1] n_valid
    void *cub_tmp;
    size_t cub_sort_bytes, cub_scan_bytes;
};

struct DOffsets {
    long long b1, w2, b2, w3, b3, w4, b4;
};
__host__ __device__ inline DOffsets d_offsets(int n_items)
{
    DOffsets o;
    o.b1 = (long long)n_items * HD;
    o.w2 = o.b1 + HD;
    o.b2 = o.w2 + HD * HD;
    o.w3 = o.b2 + HD;
    o.b3 = o.w3 + HD * HD;
    o.w4 = o.b3 + HD;
    o.b4 = o.w4 + HD;
    return o;
}
constexpr int kTail = HD + HD * HD + HD + HD * HD + HD + HD + 1;

// One block per discriminator row.  mode 0: rows [0, 2B) = real (y = 1) / fake (y = 0), forward + BCE + backward
// (d_loss = (BCE(D(real), 1) + BCE(D(fake), 0)) / 2, aush.py:147-155); the real blocks also write the batch's entry
// tables and sort keys.  mode 1: rows [0, B) = fake with y = 1, forward + BCE only (g_loss_gan, aush.py:160-161).
__global__ __launch_bounds__(256) void d_rows_kernel(int mode, int n_items, const float *__restrict__ P, DWork w,
                                                     const int *__restrict__ fcol, const float *__restrict__ fval,
                                                     const int *__restrict__ nf, const float *__restrict__ sval,
                                                     const float *__restrict__ gen, const int *__restrict__ sel)
{
    __shared__ int ec[RK_AUSH_MAX_FILLER + RK_AUSH_MAX_SELECT];
    __shared__ float ev[RK_AUSH_MAX_FILLER + RK_AUSH_MAX_SELECT];
    __shared__ float h1[HD], h2[HD], h3[HD], dz[HD], red[4];
    const DOffsets o = d_offsets(n_items);
    const int B = w.B, F = w.F, S = w.n_sel, W = F + S, j = threadIdx.x;
    const int row = blockIdx.x;
    const bool fake = mode == 1 || row >= B;
    const int b = mode == 1 ? row : (row >= B ? row - B : row);
    const float y = mode == 1 ? 1.f : (fake ? 0.f : 1.f);
    const int n = nf[b];
    // D input = profile * (fillers_mask + selects_mask) (aush.py:147-148): fillers carry the real rating (the template
    // equals the real row there); at S the real row carries its rating, the fake one gen + 5 -- target_patch is written at
    // selected_ids in training (aush.py:121,131-134).
    for (int k = j; k < W; k += blockDim.x) {
        int c;
        float vr, vf;
        if (k < F) {
            c = k < n ? fcol[(long long)b * F + k] : kSentinel;
            vr = vf = k < n ? fval[(long long)b * F + k] : 0.f;
        } else {
            c = sel[k - F];
            vr = sval[(long long)b * S + (k - F)];
            vf = gen[(long long)b * S + (k - F)] + 5.0f;
        }
        ec[k] = c;
        ev[k] = fake ? vf : vr;
        if (mode == 0 && !fake) {
            const long long e = (long long)b * W + k;
            w.ecol[e] = c;
            w.eval_r[e] = vr;
            w.eval_f[e] = vf;
            w.keys[e] = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)e;
        }
    }
    __syncthreads();
    if (j < HD) {
        float acc = 0.f;
        for (int k = 0; k < W; ++k)
            if (ec[k] != kSentinel) acc += ev[k] * P[(long long)ec[k] * HD + j];
        h1[j] = sigm(acc + P[o.b1 + j]);
    }
    __syncthreads();
    if (j < HD) {
        float acc = 0.f;
        for (int i = 0; i < HD; ++i) acc += P[o.w2 + j * HD + i] * h1[i];
        h2[j] = sigm(acc + P[o.b2 + j]);
    }
    __syncthreads();
    if (j < HD) {
        float acc = 0.f;
        for (int i = 0; i < HD; ++i) acc += P[o.w3 + j * HD + i] * h2[i];
        h3[j] = sigm(acc + P[o.b3 + j]);
    }
    __syncthreads();
    const float z4 = block_sum_256(j < HD ? P[o.w4 + j] * h3[j] : 0.f, red) + P[o.b4];
    const float x = sigm(z4);
    // torch BCELoss: each log clamped at -100
    const float l = y > 0.5f ? -fmaxf(logf(x), -100.f) : -fmaxf(log1pf(-x), -100.f);
    if (mode == 1) {
        if (j == 0) w.bce[2 * B + b] = l;
        return;
    }
    if (j == 0) w.bce[row] = l;
    // backward.  BCE: (x - y) / max(x (1 - x), 1e-12) times the upstream 0.5, / B for the mean; sigmoid: g (1 - s) s
    const float gx = (0.5f * (x - y)) / fmaxf((1.f - x) * x, 1e-12f) / (float)B;
    const float dz4 = gx * (1.f - x) * x;
    const long long rb = (long long)row * HD;
    if (j < HD) {
        w.h1[rb + j] = h1[j];
        w.h2[rb + j] = h2[j];
        w.h3[rb + j] = h3[j];
        const float d3 = dz4 * P[o.w4 + j] * (1.f - h3[j]) * h3[j];
        dz[j] = d3;
        w.dz3[rb + j] = d3;
    }
    if (j == 0) w.dz4[row] = dz4;
    __syncthreads();
    float d2 = 0.f;
    if (j < HD) {
        float acc = 0.f;
        for (int q = 0; q < HD; ++q) acc += P[o.w3 + q * HD + j] * dz[q];
        d2 = acc * (1.f - h2[j]) * h2[j];
        w.dz2[rb + j] = d2;
    }
    __syncthreads();
    if (j < HD) dz[j] = d2;
    __syncthreads();
    if (j < HD) {
        float acc = 0.f;
        for (int q = 0; q < HD; ++q) acc += P[o.w2 + q * HD + j] * dz[q];
        w.dz1[rb + j] = acc * (1.f - h1[j]) * h1[j];
    }
}

// dense-tail gradients (b1, W2, b2, W3, b3, w4, b4), one thread per parameter, rows summed in order 0..2B-1
__global__ __launch_bounds__(256) void d_tail_grad_kernel(DWork w)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= kTail) return;
    const int R = 2 * w.B;
    float acc = 0.f;
    int q = p;
    if (q < HD) {
        for (int r = 0; r < R; ++r) acc += w.dz1[(long long)r * HD + q];
    } else if ((q -= HD) < HD * HD) {
        const int a = q / HD, c = q % HD;
        for (int r = 0; r < R; ++r) acc += w.dz2[(long long)r * HD + a] * w.h1[(long long)r * HD + c];
    } else if ((q -= HD * HD) < HD) {
        for (int r = 0; r < R; ++r) acc += w.dz2[(long long)r * HD + q];
    } else if ((q -= HD) < HD * HD) {
        const int a = q / HD, c = q % HD;
        for (int r = 0; r < R; ++r) acc += w.dz3[(long long)r * HD + a] * w.h2[(long long)r * HD + c];
    } else if ((q -= HD * HD) < HD) {
        for (int r = 0; r < R; ++r) acc += w.dz3[(long long)r * HD + q];
    } else if ((q -= HD) < HD) {
        for (int r = 0; r < R; ++r) acc += w.dz4[r] * w.h3[(long long)r * HD + q];
    } else {
        for (int r = 0; r < R; ++r) acc += w.dz4[r];
    }
    w.gtail[p] = acc;
}

// segment heads of the sorted (item, entry) keys; padding entries (kSentinel item) sort last and are dropped
__global__ void seg_flag_kernel(DWork w)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= w.E) return;
    const unsigned c = (unsigned)(w.keys_sorted[e] >> 32);
    const bool valid = c != (unsigned)kSentinel;
    w.flag[e] = (valid && (e == 0 || (unsigned)(w.keys_sorted[e - 1] >> 32) != c)) ? 1 : 0;
}

__global__ void seg_start_kernel(DWork w)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= w.E) return;
    const unsigned c = (unsigned)(w.keys_sorted[e] >> 32);
    const bool valid = c != (unsigned)kSentinel;
    if (w.flag[e]) {
        w.seg_start[w.segid[e]] = e;
        w.ucol[w.segid[e]] = (int)c;
    }
    const bool last_valid = valid && (e == w.E - 1 || (unsigned)(w.keys_sorted[e + 1] >> 32) == (unsigned)kSentinel);
    if (last_valid) {
        w.counts[0] = w.segid[e] + w.flag[e];
        w.counts[1] = e + 1;
    }
    if (e == 0 && !valid) w.counts[0] = w.counts[1] = 0;
}

// first-layer gradient rows: one block per touched item, its entries in (item, row) order, real before fake
__global__ __launch_bounds__(256) void w1_grad_kernel(DWork w, unsigned char *__restrict__ touched, int *__restrict__ touched_list,
                                                      int *__restrict__ n_touched, int *__restrict__ gslot)
{
    const int s = blockIdx.x, j = threadIdx.x;
    const int n_seg = w.counts[0];
    if (s >= n_seg) return;
    const int b0 = w.seg_start[s], b1 = s + 1 < n_seg ? w.seg_start[s + 1] : w.counts[1];
    const int W = w.F + w.n_sel;
    if (j < HD) {
        float acc = 0.f;
        for (int e = b0; e < b1; ++e) {
            const int id = (int)(w.keys_sorted[e] & 0xffffffffULL);
            const int b = id / W;
            acc += w.eval_r[id] * w.dz1[(long long)b * HD + j];
            acc += w.eval_f[id] * w.dz1[(long long)(w.B + b) * HD + j];
        }
        w.gbuf[(long long)s * HD + j] = acc;
    }
    if (j == 0) {
        const int c = w.ucol[s];
        gslot[c] = s;
        if (!touched[c]) {
            touched[c] = 1;
            touched_list[atomicAdd(n_touched, 1)] = c;
        }
    }
}

// Adam (torch.optim.Adam, adam_elem) over D packed in one buffer: blocks [0, tail_blocks) the dense tail, the rest the
// first-layer rows touched so far.  A row never touched has m = v = g = 0, so its update is exactly zero and is skipped;
// a touched row is updated on every later step (g = 0 when the batch does not touch it), as torch does.
__global__ __launch_bounds__(256) void d_adam_kernel(int n_items, float *__restrict__ P, float *__restrict__ M, float *__restrict__ V,
                                                     DWork w, const int *__restrict__ touched_list, const int *__restrict__ n_touched,
                                                     const int *__restrict__ gslot, int tail_blocks, float step_size, float bc2s,
                                                     float b1, float b2, float eps)
{
    const float w1 = (float)(1.0 - (double)b1), w2 = (float)(1.0 - (double)b2);
    if ((int)blockIdx.x < tail_blocks) {
        const int p = blockIdx.x * blockDim.x + threadIdx.x;
        if (p >= kTail) return;
        const long long i = (long long)n_items * HD + p;
        float pp = P[i], mm = M[i], vv = V[i];
        adam_elem(pp, mm, vv, w.gtail[p], w1, b2, w2, step_size, bc2s, eps);
        P[i] = pp; M[i] = mm; V[i] = vv;
        return;
    }
    const long long total = (long long)(*n_touched) * HD;
    const long long stride = (long long)(gridDim.x - tail_blocks) * blockDim.x;
    for (long long t = (long long)(blockIdx.x - tail_blocks) * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int c = touched_list[t / HD], jj = (int)(t % HD);
        const int slot = gslot[c];
        const float g = slot >= 0 ? w.gbuf[(long long)slot * HD + jj] : 0.f;
        const long long i = (long long)c * HD + jj;
        float pp = P[i], mm = M[i], vv = V[i];
        adam_elem(pp, mm, vv, g, w1, b2, w2, step_size, bc2s, eps);
        P[i] = pp; M[i] = mm; V[i] = vv;
    }
}

__global__ void clear_slots_kernel(DWork w, int *__restrict__ gslot)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < w.counts[0]) gslot[w.ucol[s]] = -1;
}

// the batch's four losses, sums in a fixed order (one thread each):
//   d_loss = (mean BCE(D(real), 1) + mean BCE(D(fake), 0)) / 2, g_loss_rec = sum_ZR (gen + 5)^2 / (B I),
//   g_loss_shilling = sum gen^2 / (B I) (MSE means over the full B x I array, aush.py:162-167), g_loss_gan = mean BCE(D(fake), 1)
__global__ void d_loss_kernel(DWork w, int n_items, const float *__restrict__ gen, const unsigned char *__restrict__ zr,
                              float *__restrict__ out)
{
    const int t = threadIdx.x, B = w.B, S = w.n_sel;
    const double BI = (double)B * (double)n_items;
    if (t == 0) {
        double a = 0.0, c = 0.0;
        for (int b = 0; b < B; ++b) a += (double)w.bce[b];
        for (int b = 0; b < B; ++b) c += (double)w.bce[B + b];
        out[0] = 0.5f * ((float)(a / B) + (float)(c / B));
    } else if (t == 1) {
        double a = 0.0;
        for (int p = 0; p < B * S; ++p)
            if (zr[p]) { const double g = (double)(gen[p] + 5.0f); a += g * g; }
        out[1] = (float)(a / BI);
    } else if (t == 2) {
        double a = 0.0;
        for (int p = 0; p < B * S; ++p) { const double g = (double)gen[p]; a += g * g; }
        out[2] = (float)(a / BI);
    } else if (t == 3) {
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += (double)w.bce[2 * B + b];
        out[3] = (float)(a / B);
    }
}

// ---------------------------------------------------------------- generate_fake assembly (aush.py:187-206)
__global__ void fake_kernel(int n_rows, int n_items, int F, const int *__restrict__ fcol, const float *__restrict__ fval,
                            const int *__restrict__ nf, const int *__restrict__ sel, int n_sel, const float *__restrict__ gen,
                            const int *__restrict__ tgt, int n_tgt, float *__restrict__ pre, float *__restrict__ out)
{
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    float *o = out + (long long)r * n_items;
    for (int k = threadIdx.x; k < nf[r]; k += blockDim.x) o[fcol[(long long)r * F + k]] = fval[(long long)r * F + k];
    for (int k = threadIdx.x; k < n_tgt; k += blockDim.x) o[tgt[k]] = 5.0f;   // every target on every row
    __syncthreads();
    for (int s = threadIdx.x; s < n_sel; s += blockDim.x) {
        bool is_t = false;
        for (int k = 0; k < n_tgt; ++k) is_t |= tgt[k] == sel[s];
        const float v = gen[(long long)r * n_sel + s] + (is_t ? 5.0f : 0.0f);
        if (pre) pre[(long long)r * n_sel + s] = v;
        o[sel[s]] = fminf(fmaxf(rintf(v), 1.0f), 5.0f);   // np.round (half to even), then clip to [1, 5]
    }
}

inline long long align256(long long x) { return (x + 255) & ~255LL; }

// carve the workspace; bytes only when base == nullptr
int d_work_layout(char *base, int B, int F, int n_sel, int n_items, DWork *w, long long *bytes)
{
    DWork d{};
    d.B = B; d.F = F; d.n_sel = n_sel; d.E = B * (F + n_sel);
    const long long R = 2LL * B, E = d.E;
    long long off = 0;
    auto take = [&](long long n) { char *p = base ? base + off : nullptr; off += align256(n); return p; };
    d.h1 = (float *)take(R * HD * 4); d.h2 = (float *)take(R * HD * 4); d.h3 = (float *)take(R * HD * 4);
    d.dz1 = (float *)take(R * HD * 4); d.dz2 = (float *)take(R * HD * 4); d.dz3 = (float *)take(R * HD * 4);
    d.dz4 = (float *)take(R * 4); d.bce = (float *)take(3LL * B * 4);
    d.gtail = (float *)take((long long)kTail * 4); d.gbuf = (float *)take(E * HD * 4);
    d.ecol = (int *)take(E * 4); d.eval_r = (float *)take(E * 4); d.eval_f = (float *)take(E * 4);
    d.keys = (unsigned long long *)take(E * 8); d.keys_sorted = (unsigned long long *)take(E * 8);
    d.flag = (int *)take(E * 4); d.segid = (int *)take(E * 4); d.seg_start = (int *)take(E * 4); d.ucol = (int *)take(E * 4);
    d.counts = (int *)take(64);
    size_t sb = 0, scb = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, sb, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)E) != hipSuccess)
        return 1;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, scb, (int *)nullptr, (int *)nullptr, (int)E) != hipSuccess) return 1;
    d.cub_sort_bytes = sb; d.cub_scan_bytes = scb;
    d.cub_tmp = take((long long)std::max(sb, scb));
    (void)n_items;
    if (w) *w = d;
    *bytes = off;
    return 0;
}

int check_d(const rk_aush_desc *d)
{
    if (!d || d->n_users <= 0 || d->n_items <= 0 || d->filler_num <= 0 || d->filler_num > RK_AUSH_MAX_FILLER || d->n_sel <= 0 ||
        d->n_sel > RK_AUSH_MAX_SELECT || d->batch <= 0 || (long long)d->batch * d->n_sel > RK_AUSH_MAX_PAIRS)
        RK_FAIL(RK_EINVAL, "aush: bad sizes (n_users %d, n_items %d, filler_num %d (max %d), |S| %d (max %d), batch %d, batch*|S| max %d)",
                d ? d->n_users : 0, d ? d->n_items : 0, d ? d->filler_num : 0, RK_AUSH_MAX_FILLER, d ? d->n_sel : 0,
                RK_AUSH_MAX_SELECT, d ? d->batch : 0, RK_AUSH_MAX_PAIRS);
    if (!d->rowptr || !d->col || !d->val || !d->sel || !d->g_w1t || !d->g_b1 || !d->g_w2 || !d->g_b2 || !d->d_param || !d->d_m ||
        !d->d_v || !d->touched || !d->touched_list || !d->n_touched || !d->gslot || !d->work)
        RK_FAIL(RK_EINVAL, "aush: null pointer in the descriptor");
    return RK_OK;
}

}  // namespace

RK_EXPORT int rk_aush_workspace_bytes(int32_t batch, int32_t filler_num, int32_t n_sel, int64_t *bytes)
{
    if (batch <= 0 || filler_num <= 0 || n_sel <= 0 || !bytes) RK_FAIL(RK_EINVAL, "rk_aush_workspace_bytes: bad arguments");
    long long b = 0;
    if (d_work_layout(nullptr, batch, filler_num, n_sel, 1, nullptr, &b)) RK_FAIL(RK_EHIP, "rk_aush_workspace_bytes: hipcub sizing failed");
    *bytes = b;
    return RK_OK;
}

RK_EXPORT int rk_aush_eligible(int32_t n_users, const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *excl,
                               int32_t n_excl, int32_t filler_num, int32_t *pool_ptr, int32_t *pool_col, int32_t *eligible,
                               int32_t *n_eligible, void *stream)
{
    if (n_users <= 0 || !rowptr || !col || !val || (n_excl > 0 && !excl) || n_excl < 0 || !pool_ptr || !pool_col || !eligible || !n_eligible)
        RK_FAIL(RK_EINVAL, "rk_aush_eligible: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    int *cnt = nullptr, *flag = nullptr, *n_sel_d = nullptr;
    void *tmp = nullptr;
    size_t scan_b = 0, sel_b = 0;
    RK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (int *)nullptr, (int *)nullptr, n_users + 1, s));
    RK_HIP(hipcub::DeviceSelect::Flagged(nullptr, sel_b, (int *)nullptr, (int *)nullptr, (int *)nullptr, (int *)nullptr, n_users, s));
    RK_HIP(scratch.get(&cnt, (size_t)n_users + 1));
    RK_HIP(scratch.get(&flag, (size_t)n_users));
    RK_HIP(scratch.get(&n_sel_d, 2));
    RK_HIP(scratch.bytes(&tmp, std::max(scan_b, sel_b)));
    RK_HIP(hipMemsetAsync(cnt + n_users, 0, sizeof(int), s));
    const dim3 grid((n_users + 3) / 4);
    hipLaunchKernelGGL(pool_count_kernel, grid, dim3(256), 0, s, n_users, rowptr, col, val, excl, n_excl, cnt);
    RK_CHECK_LAUNCH();
    RK_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, scan_b, cnt, pool_ptr, n_users + 1, s));
    hipLaunchKernelGGL(pool_fill_kernel, grid, dim3(256), 0, s, n_users, rowptr, col, val, excl, n_excl, pool_ptr, pool_col,
                       filler_num, flag);
    RK_CHECK_LAUNCH();
    hipcub::CountingInputIterator<int> ids(0);
    RK_HIP(hipcub::DeviceSelect::Flagged(tmp, sel_b, ids, flag, eligible, n_sel_d, n_users, s));
    RK_HIP(hipMemcpyAsync(n_eligible, n_sel_d, sizeof(int), hipMemcpyDeviceToHost, s));
    RK_HIP(hipStreamSynchronize(s));
    return RK_OK;
}

RK_EXPORT int rk_aush_permute(int32_t n, const int32_t *in, uint64_t seed, uint64_t stream_id, int32_t *out, void *stream)
{
    if (n < 0 || (n > 0 && (!in || !out))) RK_FAIL(RK_EINVAL, "rk_aush_permute: bad arguments");
    if (n == 0) return RK_OK;
    hipStream_t s = (hipStream_t)stream;
    RkScratch scratch(s);
    unsigned long long *keys = nullptr, *ks = nullptr;
    int *pos = nullptr, *ps = nullptr;
    void *tmp = nullptr;
    size_t tb = 0;
    RK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys, ks, pos, ps, n, 0, 64, s));
    RK_HIP(scratch.get(&keys, (size_t)n));
    RK_HIP(scratch.get(&ks, (size_t)n));
    RK_HIP(scratch.get(&pos, (size_t)n));
    RK_HIP(scratch.get(&ps, (size_t)n));
    RK_HIP(scratch.bytes(&tmp, tb));
    hipLaunchKernelGGL(perm_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, (unsigned long long)seed,
                       (unsigned long long)stream_id, keys, pos);
    RK_CHECK_LAUNCH();
    RK_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys, ks, pos, ps, n, 0, 64, s));
    hipLaunchKernelGGL(gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, in, ps, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aush_sample(int32_t n_rows, const int32_t *users, int32_t filler_num, const int32_t *rowptr, const int32_t *col,
                             const float *val, const int32_t *pool_ptr, const int32_t *pool_col, const int32_t *draws, uint64_t seed,
                             uint64_t stream_id, int64_t row0, const int32_t *sel, int32_t n_sel, int32_t *fcol, float *fval, int32_t *nf,
                             float *sval, void *stream)
{
    if (n_rows < 0 || filler_num <= 0 || filler_num > RK_AUSH_MAX_FILLER || n_sel <= 0 || n_sel > RK_AUSH_MAX_SELECT || !users || !rowptr ||
        !col || !val || !sel || !fcol || !fval || !nf || !sval || (!draws && (!pool_ptr || !pool_col)))
        RK_FAIL(RK_EINVAL, "rk_aush_sample: bad arguments");
    if (n_rows == 0) return RK_OK;
    hipLaunchKernelGGL(sample_kernel, dim3(n_rows), dim3(64), 0, (hipStream_t)stream, n_rows, users, filler_num, rowptr, col, val,
                       pool_ptr, pool_col, draws, (unsigned long long)seed, (unsigned long long)stream_id, (long long)row0, sel, n_sel,
                       fcol, fval, nf, sval);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aush_zr(int32_t n_rows, int32_t batch, int32_t n_sel, const float *sval, double zr_ratio, uint64_t seed,
                         uint64_t stream_id, uint8_t *zr, void *stream)
{
    if (n_rows < 0 || batch <= 0 || n_sel <= 0 || (long long)batch * n_sel > RK_AUSH_MAX_PAIRS || !sval || !zr)
        RK_FAIL(RK_EINVAL, "rk_aush_zr: bad arguments (batch * |S| at most %d)", RK_AUSH_MAX_PAIRS);
    if (n_rows == 0) return RK_OK;
    hipLaunchKernelGGL(zr_kernel, dim3((n_rows + batch - 1) / batch), dim3(1024), 0, (hipStream_t)stream, n_rows, batch, n_sel, sval,
                       zr_ratio, (unsigned long long)seed, (unsigned long long)stream_id, zr);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aush_gen(int32_t n_rows, int32_t filler_num, const int32_t *fcol, const float *fval, const int32_t *nf,
                          const float *w1t, const float *b1, const float *w2, const float *b2, const int32_t *sel, int32_t n_sel,
                          float *gen, void *stream)
{
    if (n_rows < 0 || filler_num <= 0 || n_sel <= 0 || !fcol || !fval || !nf || !w1t || !b1 || !w2 || !b2 || !sel || !gen)
        RK_FAIL(RK_EINVAL, "rk_aush_gen: bad arguments");
    if (n_rows == 0) return RK_OK;
    hipLaunchKernelGGL(gen_kernel, dim3(n_rows), dim3(HG), 0, (hipStream_t)stream, n_rows, filler_num, fcol, fval, nf, w1t, b1, w2, b2,
                       sel, n_sel, gen);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

static int d_step(const rk_aush_desc *d, DWork &w, int32_t B, const int32_t *fcol, const float *fval, const int32_t *nf,
                  const float *sval, const float *gen, const uint8_t *zr, int32_t adam_t, float *losses, hipStream_t s)
{
    w.B = B;
    w.E = B * (d->filler_num + d->n_sel);
    const int E = w.E;
    const int end_bit = 63;   // item ids (and the padding item kSentinel = 2^31 - 1) sit in bits 32..62
    hipLaunchKernelGGL(d_rows_kernel, dim3(2 * B), dim3(256), 0, s, 0, d->n_items, (const float *)d->d_param, w, fcol, fval, nf, sval, gen,
                       d->sel);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(d_tail_grad_kernel, dim3((kTail + 255) / 256), dim3(256), 0, s, w);
    RK_CHECK_LAUNCH();
    size_t sb = w.cub_sort_bytes;
    RK_HIP(hipcub::DeviceRadixSort::SortKeys(w.cub_tmp, sb, w.keys, w.keys_sorted, E, 0, end_bit, s));
    hipLaunchKernelGGL(seg_flag_kernel, dim3((E + 255) / 256), dim3(256), 0, s, w);
    RK_CHECK_LAUNCH();
    size_t scb = w.cub_scan_bytes;
    RK_HIP(hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, scb, w.flag, w.segid, E, s));
    hipLaunchKernelGGL(seg_start_kernel, dim3((E + 255) / 256), dim3(256), 0, s, w);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(w1_grad_kernel, dim3(E), dim3(256), 0, s, w, d->touched, d->touched_list, d->n_touched, d->gslot);
    RK_CHECK_LAUNCH();
    const AdamCoef c = adam_coef(adam_t, d->lr, d->beta1, d->beta2);
    const int tail_blocks = (kTail + 255) / 256;
    hipLaunchKernelGGL(d_adam_kernel, dim3(tail_blocks + 2048), dim3(256), 0, s, d->n_items, d->d_param, d->d_m, d->d_v, w,
                       (const int *)d->touched_list, (const int *)d->n_touched, (const int *)d->gslot, tail_blocks, c.step_size, c.bc2s,
                       d->beta1, d->beta2, d->eps);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(clear_slots_kernel, dim3((E + 255) / 256), dim3(256), 0, s, w, d->gslot);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(d_rows_kernel, dim3(B), dim3(256), 0, s, 1, d->n_items, (const float *)d->d_param, w, fcol, fval, nf, sval, gen,
                       d->sel);
    RK_CHECK_LAUNCH();
    hipLaunchKernelGGL(d_loss_kernel, dim3(1), dim3(64), 0, s, w, d->n_items, gen, zr, losses);
    RK_CHECK_LAUNCH();
    return RK_OK;
}

RK_EXPORT int rk_aush_d_step(const rk_aush_desc *d, int32_t B, const int32_t *fcol, const float *fval, const int32_t *nf, const float *sval,
                             const float *gen, const uint8_t *zr, int32_t adam_t, float *losses, void *stream)
{
    if (check_d(d)) return RK_EINVAL;
    if (B <= 0 || B > d->batch || !fcol || !fval || !nf || !sval || !gen || !zr || !losses || adam_t < 1)
        RK_FAIL(RK_EINVAL, "rk_aush_d_step: bad arguments (B %d, batch %d, adam_t %d)", B, d->batch, adam_t);
    long long need = 0;
    DWork w;
    if (d_work_layout(nullptr, d->batch, d->filler_num, d->n_sel, d->n_items, nullptr, &need)) RK_FAIL(RK_EHIP, "aush: hipcub sizing failed");
    if (d->work_bytes < need) RK_FAIL(RK_EINVAL, "rk_aush_d_step: workspace %lld bytes < %lld", (long long)d->work_bytes, need);
    d_work_layout((char *)d->work, d->batch, d->filler_num, d->n_sel, d->n_items, &w, &need);
    return d_step(d, w, B, fcol, fval, nf, sval, gen, zr, adam_t, losses, (hipStream_t)stream);
}

RK_EXPORT int rk_aush_train_epoch(const rk_aush_desc *d, const int32_t *eligible, int32_t n_eligible, const int32_t *pool_ptr,
                                  const int32_t *pool_col, uint64_t seed, uint64_t epoch, double zr_ratio, int32_t adam_t0, int32_t *perm,
                                  int32_t *fcol, float *fval, int32_t *nf, float *sval, float *gen, uint8_t *zr, float *losses, void *stream)
{
    if (check_d(d)) return RK_EINVAL;
    if (n_eligible <= 0 || !eligible || !pool_ptr || !pool_col || !perm || !fcol || !fval || !nf || !sval || !gen || !zr || !losses ||
        adam_t0 < 0)
        RK_FAIL(RK_EINVAL, "rk_aush_train_epoch: bad arguments (n_eligible %d)", n_eligible);
    hipStream_t s = (hipStream_t)stream;
    long long need = 0;
    DWork w;
    if (d_work_layout(nullptr, d->batch, d->filler_num, d->n_sel, d->n_items, nullptr, &need)) RK_FAIL(RK_EHIP, "aush: hipcub sizing failed");
    if (d->work_bytes < need) RK_FAIL(RK_EINVAL, "rk_aush_train_epoch: workspace %lld bytes < %lld", (long long)d->work_bytes, need);
    d_work_layout((char *)d->work, d->batch, d->filler_num, d->n_sel, d->n_items, &w, &need);
    const int N = n_eligible, F = d->filler_num, S = d->n_sel, Bt = d->batch;
    if (int rc = rk_aush_permute(N, eligible, seed, epoch, perm, stream)) return rc;
    if (int rc = rk_aush_sample(N, perm, F, d->rowptr, d->col, d->val, pool_ptr, pool_col, nullptr, seed, epoch, 0, d->sel, S, fcol, fval,
                                nf, sval, stream))
        return rc;
    if (int rc = rk_aush_zr(N, Bt, S, sval, zr_ratio, seed, epoch, zr, stream)) return rc;
    if (int rc = rk_aush_gen(N, F, fcol, fval, nf, d->g_w1t, d->g_b1, d->g_w2, d->g_b2, d->sel, S, gen, stream)) return rc;
    const int nb = (N + Bt - 1) / Bt;
    for (int b = 0; b < nb; ++b) {
        const long long r0 = (long long)b * Bt;
        const int B = (int)std::min<long long>(Bt, N - r0);
        if (int rc = d_step(d, w, B, fcol + r0 * F, fval + r0 * F, nf + r0, sval + r0 * S, gen + r0 * S, zr + r0 * S, adam_t0 + b + 1,
                            losses + 4LL * b, s))
            return rc;
    }
    return RK_OK;
}

RK_EXPORT int rk_aush_fake_assemble(int32_t n_rows, int32_t n_items, int32_t filler_num, const int32_t *fcol, const float *fval,
                                    const int32_t *nf, const int32_t *sel, int32_t n_sel, const float *gen, const int32_t *tgt, int32_t n_tgt,
                                    float *pre, float *out, void *stream)
{
    if (n_rows < 0 || n_items <= 0 || filler_num <= 0 || n_sel <= 0 || n_tgt < 0 || !fcol || !fval || !nf || !sel || !gen ||
        (n_tgt > 0 && !tgt) || !out)
        RK_FAIL(RK_EINVAL, "rk_aush_fake_assemble: bad arguments");
    if (n_rows == 0) return RK_OK;
    hipStream_t s = (hipStream_t)stream;
    RK_HIP(rk_zero_async(out, sizeof(float) * (size_t)n_rows * (size_t)n_items, s));
    hipLaunchKernelGGL(fake_kernel, dim3(n_rows), dim3(64), 0, s, n_rows, n_items, filler_num, fcol, fval, nf, sel, n_sel, gen, tgt, n_tgt,
                       pre, out);
    RK_CHECK_LAUNCH();
    return RK_OK;
}
