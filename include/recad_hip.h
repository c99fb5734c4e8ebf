/*
 * recad_hip.h -- C ABI of librecad_hip.so, the MI355X (gfx950) implementation of RecAD's
 * victim-model hot path.  Plain pointers and sizes only; every pointer marked "device"
 * is a HIP device pointer owned by the caller (e.g. torch.Tensor.data_ptr()); `stream`
 * is a hipStream_t passed as void*.  Nothing here allocates caller-visible memory.
 *
 * The reference (gusye1234/recad v0.0.2) is pure Python on ATen: it has NO FFI for this
 * path.  Its boundary is the duck-typed victim class; each entry point
 * below names the reference code it replaces (paths under /root/reference), and
 * INTEGRATION.md shows the ctypes binding a maintainer would add to the reference.
 *
 * Return value: 0 on success, negative on error (RK_E*); rk_last_error() gives the text.
 * Thread-safety: one handle per host thread; entry points are asynchronous on `stream`
 * unless stated otherwise.
 */
#ifndef RECAD_HIP_H
#define RECAD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RK_ABI_VERSION 11
#define RK_OK 0
#define RK_EINVAL (-22)   /* bad argument / unsupported shape */
#define RK_EHIP (-5)      /* a HIP runtime call failed */
#define RK_ENOMEM (-12)

/* number of float partials rk_*_train_epoch writes per step */
#define RK_LOSS_PARTIALS 256

int rk_abi_version(void);
const char *rk_last_error(void);
/* Device sanity: returns 0 and fills name (<=255 chars) when a gfx950 device is current. */
int rk_device_info(char *name, int32_t name_len, int32_t *cu_count);

/* ---------------------------------------------------------------- graph ------------ */
/* Coalesced COO -> CSR.  Replaces the layout ATen's sparse.mm consumes: the int64 [2,nnz]
 * index tensor + fp32 values built at recad/dataset/implicit.py:320-326,295-296.
 * coo_row must be non-decreasing (torch .coalesce()).  All device pointers. */
int rk_coo_to_csr(int32_t n_rows, int64_t nnz, const int64_t *coo_row, const int64_t *coo_col,
                  const float *coo_val, int32_t *rowptr /*[n_rows+1]*/, int32_t *col /*[nnz]*/,
                  float *val /*[nnz]*/, void *stream);

/* Work schedule for rk_spmm_csr (load balance for power-law rows): every row is cut into
 * segments of <= 64 (or 128, chosen per graph) nonzeros; whole rows are packed into workgroups of 4 or 8
 * waves (best-fit decreasing), one segment per wave; a row with more segments than a workgroup has waves
 * is cut into pieces, one workgroup each, whose partial sums meet in scratch slots -- the last workgroup
 * of a row to arrive (agent-scope ticket) adds them in piece order and runs the epilogue.
 * Rows that fit one lane-group chunk (<= dim/4 nonzeros, dim in {32,64,128}) are packed 256/dim per
 * wave, one row per lane group.  Built on the host once per (graph, dim) (reads rowptr back:
 * synchronous) and only valid for SpMMs of that `dim`.  _build returns
 *   n_blocks       an opaque launch parameter (workgroup count plus flag bits) to hand back to the SpMM
 *                  entry points unchanged,
 *   n_words        the size in int32 words of the READ-ONLY device buffer `wave_desc` that _upload fills
 *                  (wave descriptors, workgroup metas, packed-row table): shareable by any number of
 *                  handles, models and streams,
 *   scratch_words  the size in int32 words (0 when the graph has no long row) of the MUTABLE scratch block
 *                  the SpMM entry points take: arrival counters + partial-sum slots of the long rows.
 *                  Caller-allocated, zero-filled once (the counters reset themselves), one block per
 *                  stream / handle: two SpMMs in flight on one schedule must not share it.
 * class_split > 0 (= n_users for the bipartite adjacency): rows < split and rows >= split are
 * scheduled separately and interleaved 4:4 over the 8 XCDs so each XCD L2 holds one table. */
typedef struct rk_schedule *rk_schedule_t;
int rk_csr_schedule_build(int32_t n_rows, const int32_t *rowptr, int32_t class_split, int32_t dim, void *stream,
                          rk_schedule_t *out, int32_t *n_blocks, int64_t *n_words, int64_t *scratch_words);
/* the same from a HOST rowptr, no HIP call (ABI 8): what the CPU tests and the sanitizer builds drive; _words copies the
 * n_words schedule words (what _upload sends to the device) into a host array */
int rk_csr_schedule_build_host(int32_t n_rows, const int32_t *rowptr_host, int32_t class_split, int32_t dim,
                               rk_schedule_t *out, int32_t *n_blocks, int64_t *n_words, int64_t *scratch_words);
/* the same with the schedule's FORM asked for: waves = waves per workgroup (0 = choose, 4, 8, 16), seg_nnz = nonzeros per segment
 * (0 = choose, 64, 128), pack = 0 (pack short rows when a quarter of the rows is short), 1 (pack every row of <= dim/4 nonzeros;
 * dims 32 / 64 / 128 only) or -1 (never); any other value is RK_EINVAL.  All zero = rk_csr_schedule_build_host, word for word.
 * The shipped builder only ever picks 4 or 8 waves by the graph's size; this entry is how the tests reach every instantiation the
 * SpMM launch dispatches to.  Graph dropout is instantiated for 4 and 8 waves: a dropout launch on a 16-wave schedule is refused. */
int rk_csr_schedule_build_host_ex(int32_t n_rows, const int32_t *rowptr_host, int32_t class_split, int32_t dim,
                                  int32_t waves, int32_t seg_nnz, int32_t pack,
                                  rk_schedule_t *out, int32_t *n_blocks, int64_t *n_words, int64_t *scratch_words);
int rk_csr_schedule_words(rk_schedule_t sched, int32_t *host_out /*[n_words]*/);
int rk_csr_schedule_upload(rk_schedule_t sched, int32_t *wave_desc, void *stream);
int rk_csr_schedule_destroy(rk_schedule_t sched);

/* D^-1/2 A D^-1/2 of the bipartite user-item graph straight into CSR, on device.
 * Replaces ImplicitData.getSparseGraph, recad/dataset/implicit.py:243-298 (scipy dok/lil).
 * r_ptr/r_idx: user->item CSR (device, item ids sorted ascending within a user).
 * Outputs: rowptr[U+I+1], col[2E], val[2E] (device).  `tmp`: int32[I+1] device scratch; the
 * transpose uses a radix sort of the edge keys with stream-ordered temporaries (hipMallocAsync). */
int rk_build_norm_adj(int32_t n_users, int32_t n_items, const int32_t *r_ptr, const int32_t *r_idx,
                      int32_t *rowptr, int32_t *col, float *val, int32_t *tmp, void *stream);

/* Y = A.X (+ add).  Replaces torch.sparse.mm(g, all_emb), recad/model/victim/lightgcn.py:107.
 * X, add (nullable), Y: device float[n_rows*dim], row-major; n_rows*dim*4 < 4 GiB.
 * X must be FINITE: the lanes of a wave that have no entry left gather row 0 of X and multiply it by zero, so an Inf / NaN in
 * X[0] reaches rows that have no entry in column 0 (torch.sparse.mm would not do that).  A non-finite row that is neither row 0
 * nor referenced by a stored entry is never read.  The same holds for rk_spmm_csr_ex and the LightGCN handle's tables.
 * scratch: device int32[scratch_words] of rk_csr_schedule_build (NULL when that was 0). */
int rk_spmm_csr(int32_t n_rows, const int32_t *rowptr, const int32_t *col, const float *val,
                const int32_t *wave_desc, int32_t n_blocks, int32_t *scratch, int32_t dim, const float *x,
                const float *add, float *y, void *stream);

/* rk_spmm_csr with every fused epilogue the LightGCN step uses, for callers that compose a step
 * themselves (the row-sharded multi-GPU trainer runs collectives between the launches).  Row r of
 * the CSR slab addresses row r of add/y/sum_in/sum_out/zero1/zero2/adam_*; x has x_rows rows.
 *   v = A.x (+ add);  y = v;  sum_out = (sum_in + v) * sum_scale;  zero1 = zero2 = 0;
 *   adam_t > 0: torch.optim.Adam step t on adam_p/m/v with gradient v (coef_scratch: device float[2]);
 *   adam_t < 0: the same with the coefficients already in coef_scratch (rk_adam_coef_advance: a device-resident step
 *   counter, for callers that replay a captured step). */
typedef struct rk_spmm_epilogue {
    const float *add;
    float *y;
    const float *sum_in;
    float *sum_out;
    float sum_scale;
    int32_t adam_t;
    float *zero1, *zero2;
    float *adam_p, *adam_m, *adam_v, *coef_scratch;
    float lr, beta1, beta2, eps;
    /* optional frontier of the gather operand: device uint32 bitmap over x's rows, bit c clear => x[c] is all zeros and
     * the entries (r, c) are skipped (first backward layer of a train step: x = dL/dlight is non-zero on the minibatch's
     * rows only).  The surviving terms keep their CSR order but are dealt to the wave's lane groups anew, so a filtered sum
     * equals the unfiltered one up to summation order (rounding, ~1e-7 relative) and is deterministic for a fixed bitmap;
     * NULL = gather everything.  rk_rows_mark_bits sets / clears the bits.  When `add` is the SAME pointer as x (t = A x + x, the
     * first backward layer), the addend of a row whose bit is clear is not read: it is zero by this contract. */
    const uint32_t *src_filter;
} rk_spmm_epilogue;
int rk_spmm_csr_ex(int32_t n_rows, const int32_t *rowptr, const int32_t *col, const float *val,
                   const int32_t *wave_desc, int32_t n_blocks, int32_t *scratch, int32_t dim, const float *x,
                   int64_t x_rows, const rk_spmm_epilogue *epi, void *stream);

/* ---- LDS-resident sliced SpMM (recad_amd/csrc/spmm_lds.h): the fast form of the same torch.sparse.mm
 * (lightgcn.py:107) for bipartite D^-1/2 A D^-1/2 graphs whose class tables fit a CU's 160 KB LDS (ml1m / Amazon-game
 * size: <= ~9 K rows per class at 4 floats per slice).  Y[:, s] = A . X[:, s] is computed per column slice: a workgroup
 * stages the source class's whole slice in LDS once and every nonzero becomes one ds_read_b128; the matrix shrinks to a
 * 16-bit column stream because A is binary: y[r] = dinv[r] * sum_c dinv[c] * x[c], dinv = deg^-1/2 (implicit.py:259-277;
 * differs from the stored-value product by rounding only, ~1e-7 relative).
 * Gathered operands use a SLICED layout: users block [dim/Su][U][Su] followed by the items block [dim/Si][I][Si]
 * (Su = 1 << lsu, Si = 1 << lsi floats); rk_lds_pack / rk_lds_unpack convert from / to row-major [U+I, dim].
 * _build reads rowptr / col / val back (synchronous), checks that the graph qualifies and returns *n_words == 0 when it
 * does not (callers then keep rk_spmm_csr); otherwise the plan goes into a 16-byte aligned READ-ONLY device buffer of
 * n_words int32 (_upload), shareable by any number of handles and streams -- the kernel has no global scratch. */
typedef struct rk_lds_info {
    int32_t n_wg, lds_bytes, lpa, lpb;        /* launch shape: workgroups, dynamic LDS bytes, lanes per entry of the two halves */
    int32_t n_users, n_items, dim, lsu, lsi;  /* sliced-layout parameters */
    int32_t chunk;                            /* chunk caps (half 0 | half 1 << 16), informational */
    int32_t wgx_ofs, dinv_ofs, perm0_ofs, perm1_ofs, mq_ofs;   /* word offsets of the plan's sections: the launches pass them as kernel arguments (ABI 8) */
    int32_t reserved;
} rk_lds_info;
typedef struct rk_lds_plan *rk_lds_plan_t;
int rk_lds_plan_build(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val /*nullable*/,
                      int32_t dim, void *stream, rk_lds_plan_t *out, int64_t *n_words, rk_lds_info *info);
/* the same from HOST arrays, no HIP call (n_cu = compute units to fill): what the CPU tests drive */
int rk_lds_plan_build_host(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                           int32_t dim, int32_t n_cu, rk_lds_plan_t *out, int64_t *n_words, rk_lds_info *info);
/* the same with the plan's FORM asked for (ABI 11): slice_items / slice_users = slice width in floats of the items / users table
 * (0 = choose, 4, 8, 16: lpa / lpb = 1, 2, 4 lanes per entry), chunk_cap = 0 (choose), 64, 96, 128, 256, 512; any other value is
 * RK_EINVAL.  A width that does not divide dim, or a form that does not fit a CU's LDS, gives *n_words == 0 like a graph that
 * does not qualify.  All zero = rk_lds_plan_build_host, word for word.  The shipped planner only ever picks one form; this entry
 * is how the tests reach every instantiation rk_spmm_lds dispatches to (lpa, lpb: (1,1) (1,2) (2,1) (2,2) (4,4) (4,2) (2,4)). */
int rk_lds_plan_build_host_ex(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                              int32_t dim, int32_t n_cu, int32_t slice_items, int32_t slice_users, int32_t chunk_cap,
                              rk_lds_plan_t *out, int64_t *n_words, rk_lds_info *info);
int rk_lds_plan_words(rk_lds_plan_t plan, int32_t *host_out /*[n_words]*/);
int rk_lds_plan_upload(rk_lds_plan_t plan, int32_t *dev /*[n_words], 16-byte aligned*/, void *stream);
int rk_lds_plan_destroy(rk_lds_plan_t plan);
/* n_arrays arrays of (U+I)*dim floats, `stride` floats apart, converted in one launch */
int rk_lds_pack(const rk_lds_info *info, const float *row_major, float *sliced, int32_t n_arrays, int64_t stride, void *stream);
int rk_lds_unpack(const rk_lds_info *info, const float *sliced, float *row_major, int32_t n_arrays, int64_t stride, void *stream);
/* v = A.x (+ add); y = v; sum_out = (sum_in + v) * sum_scale; zero1 = zero2 = 0; Adam as in rk_spmm_csr_ex.
 * x, add, sum_in, zero1, zero2, adam_shadow: sliced.  y / sum_out: sliced unless their *_row_major flag is set.
 * adam_p / m / v: row-major; adam_shadow (nullable) receives a sliced copy of the updated parameters. */
typedef struct rk_lds_epilogue {
    const float *add;
    float *y;
    const float *sum_in;
    float *sum_out;
    float sum_scale;
    int32_t y_row_major, sum_out_row_major, adam_t;
    float *zero1, *zero2;
    float *adam_p, *adam_m, *adam_v, *adam_shadow, *coef_scratch;
    float lr, beta1, beta2, eps;
    uint64_t *stamps;   /* diagnostic, nullable: device uint64[4 * n_wg], wall-clock stamps (start, staged, gathered, done) per workgroup */
} rk_lds_epilogue;
int rk_spmm_lds(const rk_lds_info *info, const int32_t *plan, const float *x, const rk_lds_epilogue *epi, void *stream);

/* The row-sharded trainer's per-step index work (the reference's getEmbedding gathers, lightgcn.py:122-130, split over ranks):
 * out[i, :] = mask[i] * src[idx[i], :] (mask NULL = 1; a zero mask entry gives exact zeros), and a[idx[i], :] = b[idx[i], :] = 0
 * (b nullable).  idx: device int64[n]. */
int rk_rows_gather_masked(int32_t dim, const float *src, const int64_t *idx, const float *mask, int64_t n, float *out, void *stream);
int rk_rows_zero(int32_t dim, float *a, float *b, const int64_t *idx, int64_t n, void *stream);
/* bits[idx[i] >> 5] |= 1 << (idx[i] & 31) (set != 0), or the words holding those bits = 0 (set == 0) */
int rk_rows_mark_bits(uint32_t *bits, const int64_t *idx, int64_t n, int32_t set, void *stream);

/* counter[0] += 1; coef = {lr / (1 - beta1^t), sqrt(1 - beta2^t)} for t = the new counter value (device int32 / float[2]). */
int rk_adam_coef_advance(float *coef, int32_t *counter, float lr, float beta1, float beta2, void *stream);

/* BPR forward+backward of ONE minibatch on explicit node rows (lightgcn.py:122-165): rows_u/p/n
 * index emb/gprop/gego directly (item rows already offset), and light too unless light_compact != 0:
 * then light is a compact [3*nb, dim] block holding the propagated rows of the minibatch in the order
 * users, positives, negatives (triplet b reads rows b, nb+b, 2nb+b) -- what the row-sharded trainer
 * assembles with one small all-reduce instead of all-gathering the whole light table.
 * gprop += dL/dlight / (L+1), gego += that + the L2-reg gradient; loss_partials: device
 * float[RK_LOSS_PARTIALS] (every entry is written). */
int rk_bpr_rows(int32_t dim, int32_t n_layers, float lambda, const float *light, int32_t light_compact,
                const float *emb, float *gprop, float *gego, const int64_t *rows_u, const int64_t *rows_p,
                const int64_t *rows_n, int32_t nb, float *loss_partials, void *stream);

/* The same minibatch with the ordered scatter of rk_lightgcn_set_deterministic (no atomics: plain stores, one wave per
 * touched row; gprop / gego must be zero on the minibatch's rows): light is always the compact [3*nb, dim] block, and
 * keys = device uint64[3*nb], the batch's incidences (row << 20) | (3*b + role) with row < 2^24, role 0/1/2 = user/positive/negative,
 * SORTED ascending -- the caller's sort (the row-sharded trainer sorts a whole epoch with one batched torch.sort).
 * Every rank that runs it on the same triplets gets bit-identical gradient rows. */
int rk_bpr_rows_ordered(int32_t dim, int32_t n_layers, float lambda, const float *light, const float *emb, float *gprop,
                        float *gego, const int64_t *rows_u, const int64_t *rows_p, const int64_t *rows_n, int32_t nb,
                        const uint64_t *keys, float *loss_partials, void *stream);

/* ---------------------------------------------------------------- LightGCN --------- */
typedef struct rk_lightgcn_desc {
    int32_t n_users, n_items, dim, n_layers;
    float lambda, lr, beta1, beta2, eps;      /* default.py:105-115; torch.optim.Adam defaults */
    int32_t reserved0;
    /* normalised adjacency, CSR over N = n_users + n_items nodes (device) */
    const int32_t *rowptr, *col;
    const float *val;
    const int32_t *wave_desc;                 /* from rk_csr_schedule_upload */
    int32_t n_blocks, reserved1;
    /* parameters and Adam moments, row-major fp32 (device); updated in place.  The item
     * block must directly follow the user block (item_emb == user_emb + n_users*dim, same for
     * m/v): E0 = [users; items] is then ONE [N,dim] matrix and torch.cat (lightgcn.py:88) is
     * a no-op. */
    float *user_emb, *item_emb;               /* embedding_user/.item.weight, lightgcn.py:40-45 */
    float *m_user, *v_user, *m_item, *v_item; /* exp_avg / exp_avg_sq of torch.optim.Adam */
    /* workspace, each float[N*dim] (device) */
    float *buf_a, *buf_b, *light, *gprop, *gego;
    float *grad;                              /* nullable: receives dLoss/dE0 [N*dim] */
    int32_t *state;                           /* device int32[16], 8-byte aligned, owned by the handle's user */
    float *coef;                              /* device float[2*RK_MAX_GRAPH_STEPS] (3*RK_MAX_GRAPH_STEPS with cnt) */
    int32_t *spmm_scratch;                    /* int32[scratch_words] of rk_csr_schedule_build, zero-filled, owned by this
                                               * handle's user (NULL when scratch_words == 0) */
    /* optional: device uint32[(N+31)/32] bitmap of the current minibatch's rows; when given (and
     * n_layers >= 2) the last forward layer computes only those rows of `light` */
    uint32_t *row_bits;
    /* optional graph dropout of the TRAINING propagation (lightgcn.py:62-80,91-95; config keys dropout /
     * keep_prob): keep_prob in (0,1) enables it (0 = off).  Every stored entry of the adjacency is kept with
     * probability keep_prob and divided by it, one fresh mask per train step (counter-based RNG of drop_seed,
     * the step index and the entry's position: the stream differs from torch.rand, the distribution does
     * not).  The mask is drawn per stored entry, so the propagated graph is not symmetric and the backward
     * applies its transpose: tpos[e] = position of the entry (col[e], row(e)) (device int32[nnz]). */
    float keep_prob;
    int32_t reserved3;
    uint64_t drop_seed;
    const int32_t *tpos;
    /* optional LDS-resident propagation (rk_lds_plan_*): lds_plan != NULL switches every SpMM of this handle to
     * rk_spmm_lds's kernel (not with graph dropout).  buf_a / buf_b / gprop / gego then hold SLICED data (same sizes),
     * lsum, e0s, ms, vs are four more float[N*dim] work buffers: the running layer sum and the SLICED working copies of
     * E0 and the Adam moments -- refreshed from user_emb / m_user / v_user at the start of every train_epoch call (e0s
     * also by propagate), updated by the fused Adam, written back to the row-major tensors at the end of the call.
     * row_bits is unused. */
    const int32_t *lds_plan;
    rk_lds_info lds_info;
    float *lsum, *e0s, *ms, *vs;
    int32_t *cnt;                             /* optional, int32[N]: per-node incidence counts of the minibatch; with it the L2-reg
                                               * gradient is applied in closed form (lambda / nb * count * E0) and the BPR kernel
                                               * scatters three rows per triplet instead of six; coef must then hold
                                               * 3 * RK_MAX_GRAPH_STEPS floats */
    int32_t *row_blocks;                      /* optional (ABI 9, row-gather path, with row_bits and n_layers >= 3): int32[4 + number of
                                               * schedule blocks], this handle's own: word 0 counts, words 4.. list the workgroups of
                                               * the schedule that hold a row of the current minibatch, so that the row-filtered last
                                               * forward layer starts min(n_blocks, 3 * batch + row_blocks_extra) workgroups instead of
                                               * all of them (csrc/spmm.h SpmmArgs::blk_mode) */
    int32_t row_blocks_extra, reserved4;      /* upper bound of the schedule's long-row pieces (scratch_words / dim is one) */
    int32_t *lds_sync;                        /* optional (ABI 8), int32[RK_LDS_SYNC_WORDS], zero-initialised, this handle's own: with
                                               * it the L propagation layers of a forward / backward pass run as ONE launch (<= 4
                                               * layers per launch) whose workgroups hand the layers over to each other per column
                                               * group through agent-scope counters kept here (recad_amd/csrc/spmm_lds.h:
                                               * spmm_lds_multi_kernel; same sums, same bits as one launch per layer).  Word
                                               * RK_LDS_SYNC_ERR is set if a wait ever gave up and stays set until rk_lightgcn_sync_status reads it. */
} rk_lightgcn_desc;
#define RK_LDS_SYNC_WORDS 2560
#define RK_LDS_SYNC_ERR 2336
#define RK_MAX_GRAPH_STEPS 64

typedef struct rk_lightgcn *rk_lightgcn_t;

int rk_lightgcn_create(const rk_lightgcn_desc *desc, rk_lightgcn_t *out);
/* *status = desc.lds_sync[RK_LDS_SYNC_ERR] (0 = every in-launch hand-off completed; no lds_sync: 0).  Synchronises the stream.
 * The word is STICKY: no launch and no call prologue clears it (the caller's zero-initialisation and this call are the only
 * resets), so a time-out in any propagate / train call since the last status read is reported; a non-zero status is
 * cleared by the read. */
int rk_lightgcn_sync_status(rk_lightgcn_t h, int32_t *status, void *stream);
int rk_lightgcn_destroy(rk_lightgcn_t h);

/* LightGCN.computer(), recad/model/victim/lightgcn.py:82-113: desc.light[N,dim] =
 * mean_l(A^l [U;I]).  Users are rows [0,U), items rows [U,N). */
int rk_lightgcn_propagate(rk_lightgcn_t h, void *stream);
/* The same through a dropped-out graph (computer() of a module in training mode with dropout > 0,
 * lightgcn.py:91-95): mask_seed picks the mask; requires desc.keep_prob > 0. */
int rk_lightgcn_propagate_dropout(rk_lightgcn_t h, uint64_t mask_seed, void *stream);

/* One epoch of LightGCN.train_step, recad/model/victim/lightgcn.py:137-169, over the
 * pre-sampled triplets (device int64[n], the tensors ImplicitData.generate_batch yields,
 * recad/dataset/implicit.py:416-437): ceil(n/batch) steps of forward, BPR loss + L2 reg,
 * backward, dense Adam.  adam_t0 = optimizer steps already taken.  loss_partials: device
 * float[ceil(n/batch)*RK_LOSS_PARTIALS]; step s's loss is the sum of its RK_LOSS_PARTIALS
 * entries (fixed order => reproducible).  apply_update=0 leaves parameters untouched and
 * only fills desc.grad (testing).
 * graph_steps > 1 replays captured hipGraphs: an epoch of <= RK_MAX_GRAPH_STEPS steps is ONE replay of a whole-call graph
 * (scatter-target zeroing and, on the LDS path, the layout conversions included); a longer one is replayed in chunks of
 * graph_steps steps plus one remainder graph (a single trailing step is launched kernel by kernel).  The triplet and loss
 * pointers reach the kernels through desc.state, not through the captured launches, so the graphs (cached per handle, 8
 * LRU slots) serve any buffers; they must stay valid until the stream has run the call. */
int rk_lightgcn_train_epoch(rk_lightgcn_t h, const int64_t *users, const int64_t *pos, const int64_t *neg,
                            int64_t n, int32_t batch, int32_t adam_t0, float *loss_partials,
                            int32_t apply_update, int32_t graph_steps, void *stream);

/* Optional: capture, instantiate and upload ahead of time the hipGraphs that an epoch of n triplets in batches of `batch`
 * will replay, so that no epoch (or timed region) pays for it.  The reference has no counterpart (its step is eager ATen,
 * lightgcn.py:137-169). */
int rk_lightgcn_prepare(rk_lightgcn_t h, int64_t n, int32_t batch, int32_t apply_update, int32_t graph_steps, void *stream);

/* Ordered (reproducible) gradient scatter for rk_lightgcn_train_epoch.  The reference scatters the minibatch's embedding
 * gradients through autograd's index_select backward (lightgcn.py:124-129,166): a sequential sum on CPU, float atomics on a
 * GPU.  Default here: float atomics too (sum order not fixed; the loss is reproducible, gradients to ~1e-7).  on != 0:
 * train_epoch first sorts the epoch's 3n (node row, triplet, role) incidences once (handle-owned buffers, 48 bytes per
 * triplet) and every step adds each row's contributions in (triplet index, role) order with plain stores, one wave per
 * touched row instead of one per triplet -- bit-identical gradients and parameters from run to run (+5 % per ml1m step).  Limits: < 2^20 steps per epoch, < 2^24 node
 * rows, batch < 349 525.  Not used by rk_bpr_rows (the row-sharded trainer). */
int rk_lightgcn_set_deterministic(rk_lightgcn_t h, int32_t on);

/* ---------------------------------------------------------------- shared ops ------- */
/* out[b] = <utab[users[b]], itab[items[b]]> (+ ubias[users[b]] + ibias[items[b]] + mean when
 * ubias != NULL).  LightGCN.forward tail (lightgcn.py:179-182) and MF.forward (mf.py:40-47). */
int rk_pair_scores(int32_t dim, const float *utab, const float *itab, const float *ubias, const float *ibias,
                   float mean, const int64_t *users, const int64_t *items, int64_t n, float *out, float dropout,
                   uint64_t drop_seed, void *stream);   /* dropout > 0: nn.Dropout on the score (mf.py:47), mask of drop_seed */

/* Dense torch.optim.Adam step on one tensor (recad/utils.py:181-183): t = 1-based step. */
int rk_adam_step(int64_t n, float *param, const float *grad, float *m, float *v, int32_t t, float lr,
                 float beta1, float beta2, float eps, void *stream);
/* the same, coefficients {lr / (1 - beta1^t), sqrt(1 - beta2^t)} from device float[2] (rk_adam_coef_advance): for captured steps (ABI 8) */
int rk_adam_step_dev(int64_t n, float *param, const float *grad, float *m, float *v, const float *coef, float beta1, float beta2, float eps,
                     void *stream);

/* Full-catalog scoring + top-K + target rank for a block of users: replaces the per-user
 * loop of Normal.user_item_model_generate, recad/workflow/normal.py:57-93.
 *   scores[b,i] = <utab[user_ids[b]], itab[i]> (+ ubias[user_ids[b]] + ibias[i] + mean when ibias != NULL)
 * computed with fp32 MFMA (utab/ubias are the whole user tables: the block's rows are gathered on the way
 * in); items in the user's seen list (CSR seen_ptr/seen_idx indexed by user_ids[b], ids sorted ascending)
 * are excluded (normal.py:133-143).  Outputs per user: top_ids/top_scores[K] sorted by (score desc, item id
 * asc), padded with -1/-inf; for each target t its score and rank among the unseen items (hit@k <=> rank < k).
 * Scores are ranked by one key (score_panel.h score_key): -0.0 ties with +0.0, -inf and negative NaNs are in no list and count in
 * no rank, a positive NaN ranks above +inf.  The panel path requires finite tables: it compares scores as floats, so a positive
 * NaN score is in none of its lists and counts in none of its ranks; scores that overflow to +-inf from finite tables are ranked
 * alike on both paths.  A caller that cannot vouch for its tables asks for RK_SCORE_GEMM (recad_amd.evaluate checks them once per
 * evaluation when the plan took the panel path).
 * Two paths, identical results on finite tables (ids, scores, target scores and ranks bit for bit):
 *   RK_SCORE_GEMM  -- GEMM into a [nb, n_items] matrix (row stride plan.ld_scores) in `scratch` + a selection pass: small user blocks, catalogues of < 16 384
 *                     items, and everything the panel form does not take;
 *   RK_SCORE_PANEL -- the register-resident panel form, recad_amd/csrc/score_panel.h: a workgroup holds the scores of 16 / 32
 *                     users x 1920 items in its registers, selects from there and never writes a score (K <= 256, n_targets <= 4,
 *                     dim <= 256; scratch = a k-permuted copy of the item table, n_items * 16 * ceil(dim / 16) floats).  It
 *                     parallelises over the users only, so it is the default from 16 384 items on for blocks of >= 8192 users
 *                     (>= 4096 at dim <= 64).
 * The path is an ARGUMENT, not process state (ABI 8): rk_score_topk_plan() fills a plan for one (nb, n_items, dim, K, n_targets) --
 * the library's choice when request is NULL / request->path == RK_SCORE_AUTO, the requested path and shape knobs otherwise
 * (RK_EINVAL if that path does not support the request) -- with the scratch it needs, and rk_score_topk() runs exactly that plan:
 * sizing and launch cannot disagree.  (Round 2's fused sweep, score_select.h, is gone: measured slower than both paths on every
 * shape, its last default corner included -- profiles/r04_score_corner.txt.) */
#define RK_SCORE_AUTO 0
#define RK_SCORE_GEMM 1
#define RK_SCORE_PANEL 2
typedef struct rk_score_plan {
    int32_t path;             /* RK_SCORE_GEMM / RK_SCORE_PANEL (RK_SCORE_AUTO only in a request) */
    int32_t panel_rows;       /* PANEL: 16 or 32 user rows per workgroup (request: 0 = by shape) */
    int32_t panel_ntw;        /* PANEL: 16-item tiles per wave and panel: 8 (1024-item panels) or 15 (1920) (request: 0 = by catalogue size) */
    int32_t panel_safe;       /* PANEL: 1 = every panel through the exact safe form (tests) */
    int32_t nb, n_items, dim, K, n_targets;   /* what the plan was made for: rk_score_topk refuses anything else */
    int32_t ld_scores;        /* GEMM (ABI 9): row stride of the score matrix in floats = n_items rounded up to 32, so that every row and every
                               * 16-column store segment of the GEMM's tiles starts on a 128- / 64-byte line (3 702 -> 3 712); PANEL: 0 */
    int32_t reserved[2];
    int64_t scratch_floats;   /* device float[scratch_floats], 16-byte aligned (GEMM: nb * ld_scores) */
} rk_score_plan;
int rk_score_topk_plan(int32_t nb, int32_t n_items, int32_t dim, int32_t K, int32_t n_targets, const rk_score_plan *request /*nullable*/,
                       rk_score_plan *out);
int rk_score_topk(int32_t dim, const float *utab, int32_t nb, const int32_t *user_ids, const float *itab,
                  int32_t n_items, const float *ubias, const float *ibias, float mean,
                  const int32_t *seen_ptr, const int32_t *seen_idx, int32_t K, int32_t *top_ids,
                  float *top_scores, const int32_t *targets, int32_t n_targets, float *target_score,
                  int32_t *target_rank, const rk_score_plan *plan, float *scratch, void *stream);

/* ---------------------------------------------------------------- MF --------------- */
/* One epoch of MF.train_step, recad/model/victim/mf.py:49-69: logits (mf.py:40-47),
 * BCE-with-logits (mf.py:32,59-60), backward, dense Adam on the four tables.
 * grads: device float[U*d + I*d + U + I] scratch (zeroed by the call).
 * moments: m then v, same layout as grads, each [U*d + I*d + U + I]. */
int rk_mf_train_epoch(int32_t n_users, int32_t n_items, int32_t dim, float *user_emb, float *item_emb,
                      float *user_bias, float *item_bias, float mean, float *m, float *v, float *grads,
                      const int64_t *users, const int64_t *items, const int64_t *labels, int64_t n,
                      int32_t batch, int32_t adam_t0, float lr, float beta1, float beta2, float eps,
                      float *loss_partials, int32_t apply_update, float dropout, uint64_t drop_seed, void *stream);
/* dropout > 0: nn.Dropout on the logit (mf.py:27,47), one counter-based mask per optimizer step and sample. */

/* ---------------------------------------------------------------- samplers ---------- */
/* BPR triplets with the semantics of pairwise_sample, recad/dataset/implicit.py:50-74: n_draws
 * uniform user draws with replacement; a user without positives yields valid=0 (the reference
 * skips the draw); positive uniform over the user's list; negative uniform over the items NOT in
 * it.  pos_ptr/pos_idx: user->sorted item ids (device int32).  Counter-based RNG of `seed`. */
int rk_bpr_sample(int32_t n_users, int32_t n_items, const int32_t *pos_ptr, const int32_t *pos_idx,
                  int64_t n_draws, uint64_t seed, int64_t *users, int64_t *pos, int64_t *neg, int32_t *valid,
                  void *stream);

/* (user, item, label) rows of pointwise_sample, recad/dataset/implicit.py:77-91: each train edge
 * once with label 1, followed by negative_ratio rows with label 0 whose item is uniform (with
 * replacement) over the user's non-interacted items.  Outputs: int64[n_edges*(negative_ratio+1)].
 * A user who has interacted with every item has no such item: its negative rows hold (user, item 0, label 0) and are
 * the caller's to discard (ImplicitData._device_epoch does); the reference cannot draw one either. */
int rk_pointwise_sample(int32_t n_users, int32_t n_items, const int32_t *train_ptr, const int32_t *train_idx,
                        int64_t n_edges, int32_t negative_ratio, uint64_t seed, int64_t *users, int64_t *items,
                        int64_t *labels, void *stream);

/* Pass 2 of rk_score_topk on a ready score matrix scores[nb, n_items] (rows too long to stage
 * in LDS are modified in place: seen items are overwritten with -inf).  Used for victims whose
 * scores are not a dot product (NCF). */
int rk_topk_rows(float *scores, int32_t nb, int32_t n_items, const int32_t *user_ids, const int32_t *seen_ptr,
                 const int32_t *seen_idx, int32_t K, int32_t *top_ids, float *top_scores,
                 const int32_t *targets, int32_t n_targets, float *target_score, int32_t *target_rank,
                 void *stream);

/* HR@k numerators (normal.py:86-92,150-156: hit@k <=> the target's rank among the unseen items < k):
 * counts[t*nk + q] = #{b < n : target_rank[b*n_targets + t] < ks[q]}.  All pointers on the device. */
int rk_hit_counts(const int32_t *target_rank, int64_t n, int32_t n_targets, const int32_t *ks, int32_t nk,
                  int32_t *counts, void *stream);

/* Users the reference evaluates (normal.py:133-143): every user whose train list (CSR seen_ptr/seen_idx, item ids
 * sorted) is non-empty and holds none of the targets.  user_ids[0..count) = their ids in ascending order; all
 * pointers on the device; flags_scratch: int32[n_users]; count: int32[1]. */
int rk_eligible_users(int32_t n_users, const int32_t *seen_ptr, const int32_t *seen_idx, const int32_t *targets,
                      int32_t n_targets, int32_t *flags_scratch, int32_t *user_ids, int32_t *count, void *stream);

/* pred_shift (normal.py:147-149): out[0] = mean(score_after[i] - score_before[i]), out[1] = the sum, i < n, in
 * double, fixed summation order.  out: device double[2]. */
int rk_pred_shift(const float *score_before, const float *score_after, int64_t n, double *out, void *stream);

/* Held-out ranking quality of the lists rk_score_topk / rk_topk_rows wrote: what BaseTrainer.evaluate_epoch
 * (recad/model/attacker/aia.py:327-358) walks `metrics` for -- the reference's `metrics` is None, so it has no metric
 * function -- over the validate / test batches of recad/dataset/implicit.py:462-476, with the conventions of the LightGCN
 * evaluation code the victim descends from.  top_ids[n, K]: row b is the list of user user_ids[b], -1 pads match nothing;
 * gt_ptr / gt_idx: CSR of the held-out split indexed by USER ID, item ids ascending and unique within a row (an item that
 * is also in the user's seen list can never be recommended and still counts in |gt|); ks[nk]: cut-offs in any order,
 * nk <= 8, clamped to [1, K]; discount[K] = 1 / log2(j + 2) in double (the device evaluates no logarithm).
 * Per user (every element written): hits[n, nk] = held-out items among the first ks[q] entries, dcg[n, nk] = the sum of
 * discount[j] over the hit positions j < ks[q], first[n] = position of the first hit among the K entries or -1; a row with
 * an empty held-out list gets zeros and -1.
 * out[1 + 5 nk]: out[0] = rows with a non-empty held-out list; then for each q the SUMS over those rows of
 * recall = hits / |gt|, precision = hits / ks[q], ndcg = dcg / sum_{j < min(ks[q], |gt|)} discount[j], hit = [hits > 0],
 * mrr = first in [0, ks[q]) ? 1 / (first + 1) : 0 -- the caller divides by out[0].  Double, fixed summation order.
 * All pointers on the device; two launches on `stream`, no synchronisation, no allocation (capturable).  n == 0: out is
 * zeroed and nothing else is touched.  RK_EINVAL, nothing launched: n < 0 or n > INT_MAX (rows are indexed in int32),
 * K outside [1, 256], nk outside [1, 8], a null `out` (also when n == 0: it is the one buffer still written), any other
 * null pointer when n > 0. */
int rk_rank_metrics(const int32_t *top_ids, int64_t n, int32_t K, const int32_t *user_ids, const int32_t *gt_ptr,
                    const int32_t *gt_idx, const int32_t *ks, int32_t nk, const double *discount, int32_t *hits, double *dcg,
                    int32_t *first, double *out, void *stream);

/* out[b*n_items + i] = <utab[user_ids[b]], itab[i]> (+ ubias[user_ids[b]] + ibias[i] + mean), optionally through
 * nn.Dropout(dropout) on the score -- MF.forward of a module in training mode (mf.py:40-47); feeds rk_topk_rows. */
int rk_score_matrix(int32_t dim, const float *utab, int32_t nb, const int32_t *user_ids, const float *itab,
                    int32_t n_items, const float *ubias, const float *ibias, float mean, float dropout,
                    uint64_t drop_seed, float *out, void *stream);

/* LightGCN.getUsersRating (lightgcn.py:115-120): out[b*n_items + i] = sigmoid(<utab[user_ids[b]], itab[i]>), the
 * dot product on the fp32 MFMA GEMM (bit-identical to the k-ordered fmaf chain). */
int rk_users_rating(int32_t dim, const float *utab, int32_t nb, const int32_t *user_ids, const float *itab,
                    int32_t n_items, float *out, void *stream);

/* ---------------------------------------------------------------- NCF -------------- */
#define RK_NCF_MAX_LAYERS 8
#define RK_NCF_MAX_TENSORS 24
/* NCF (recad/model/victim/ncf.py:9-58; variants: `mode` below).  E = factor * 2^(n_layers-1) is the MLP embedding
 * width; tower layer l is Linear(in_l -> in_l/2) + ReLU with in_l = factor * 2^(n_layers-l)
 * (ncf.py:41-47); W[l] is nn.Linear's [out, in] row-major weight.  Tensor order of grad/m/v:
 * ug, ig, um, im, W[0..L-1], b[0..L-1], pw, pb. */
typedef struct rk_ncf_desc {
    int32_t n_users, n_items, factor, n_layers;
    float lr, beta1, beta2, eps;
    float *ug, *ig, *um, *im;                  /* embed_{user,item}_{GMF,MLP}.weight */
    float *W[RK_NCF_MAX_LAYERS], *b[RK_NCF_MAX_LAYERS];
    float *pw, *pb;                            /* predict_layer.weight [2*factor] (GMF part first), .bias [1] */
    float *grad[RK_NCF_MAX_TENSORS], *m[RK_NCF_MAX_TENSORS], *v[RK_NCF_MAX_TENSORS];
    float *acts, *dacts;                       /* each float[max_batch * sum_{l=0..L} in_l] */
    float *d0;                                 /* float[max_batch] */
    int32_t max_batch, reserved;
    /* K-slice workspace.  (1) backward (dX) tower GEMMs whose whole-K tiling would not fill the chip (batch 1024 against a
     * few hundred outputs): K-slices park partial products here and are added in slice order (deterministic); optional
     * for that.  (2) REQUIRED by rk_ncf_train_epoch when a tower layer's input width is a multiple of 256: the training
     * forward of such a layer sums its products in 8 consecutive k-blocks combined pairwise (ATen-like error: the ReLU
     * gates it decides are the masks of the backward; csrc/ncf.hip gemm_fwd_blocked, oracle ncf_forward_one_ex), the blocks
     * parked here as [8][rows, out] -- 8 * max_batch * (widest layer output) floats run every layer in one piece, less
     * makes row chunks (>= 8 * 64 * out).  rk_ncf_forward (scoring) keeps the single k-ordered chain. */
    float *gemm_scratch;
    int64_t gemm_scratch_floats;
    float *wgrad_part;                         /* training: float[ceil(max_batch/64) * (2*factor + 1)] */
    /* model variant (ncf.py:49-52,112-131): RK_NCF_NEUMF = 'NeuMF-end' / 'NeuMF-pre' (they differ in initialisation
     * only, ncf.py:78-110), RK_NCF_MLP = tower only, RK_NCF_GMF = element-wise product only; pw has 2*factor entries
     * for NeuMF and factor entries otherwise.  Tensors a variant does not use receive zero gradients. */
    int32_t mode;
    /* nn.Dropout(p) in front of every tower layer (ncf.py:44); 0 = off.  Counter-based masks of drop_seed, the call
     * (train: optimizer step; rk_ncf_forward: drop_call and the chunk) and the layer: the stream differs from
     * torch's, the distribution does not.  The reference's workflows score WITHOUT .eval() (normal.py:61-67), so a
     * module in training mode passes its dropout here for rk_ncf_forward too. */
    float dropout;
    uint64_t drop_seed;
    int32_t drop_call, reserved2;
} rk_ncf_desc;
#define RK_NCF_NEUMF 0
#define RK_NCF_MLP 1
#define RK_NCF_GMF 2

/* NCF.forward (ncf.py:112-131) for n pairs -> out[n].  Pairs are (users[b], items[b]), or -- when
 * user_ids != NULL -- the full catalog of each listed user: pair q = (user_ids[q / n_items_catalog],
 * q % n_items_catalog), which is how the evaluation fills a [users, items] score matrix. */
int rk_ncf_forward(const rk_ncf_desc *desc, const int64_t *users, const int64_t *items,
                   const int32_t *user_ids, int32_t n_items_catalog, int64_t n, float *out, void *stream);

/* One epoch of NCF.train_step (ncf.py:133-153): forward, BCE-with-logits, backward through the
 * tower (fp32 MFMA GEMMs), embedding scatter-add, dense Adam on every tensor. */
int rk_ncf_train_epoch(const rk_ncf_desc *desc, const int64_t *users, const int64_t *items,
                       const int64_t *labels, int64_t n, int32_t batch, int32_t adam_t0,
                       float *loss_partials, int32_t apply_update, void *stream);

/* ---------------------------------------------------------------- fp32 MFMA GEMM (test and diagnostic entry) */
/* The kernel instantiations behind the library's one GEMM dispatcher (csrc/gemm.h gemm_f32_launch), as rk_gemm_f32 reports them. */
#define RK_GEMM_FORM_NONE 0
#define RK_GEMM_SKINNY 1                 /* gemm_f32_skinny_kernel: 64-tiles, 32-deep chunks, bounds-checked */
#define RK_GEMM_DEEP_11_64 2             /* gemm_f32_skinny_deep_kernel<MA, MB, BM>: A and B k-contiguous */
#define RK_GEMM_DEEP_12_64 3             /*   B row-contiguous (dX) */
#define RK_GEMM_DEEP_22_64 4             /*   A and B row-contiguous (dW) */
#define RK_GEMM_DEEP_11_32 5
#define RK_GEMM_DEEP_12_32 6
#define RK_GEMM_DEEP_22_32 7
#define RK_GEMM_WIDE_11 8                /* gemm_f32_wide_kernel<1, 1> */
#define RK_GEMM_WIDE_12 9                /* gemm_f32_wide_kernel<1, 2> */
#define RK_GEMM_WIDE_11_PLAIN 10         /* gemm_f32_wide_kernel<1, 1, PLAIN> */
#define RK_GEMM_WIDE_11_PLAIN_GROUPED 11 /* gemm_f32_wide_kernel<1, 1, PLAIN, GROUPED> */
#define RK_GEMM_TILE128 12               /* gemm_f32_kernel<128, 1, 3> */
#define RK_GEMM_TILE128_GATHER 13        /* gemm_f32_kernel<128, 1, 3, GATHER> */
#define RK_GEMM_TILE128_GATHER_PLAIN 14  /* gemm_f32_kernel<128, 1, 3, GATHER, PLAIN> */
#define RK_GEMM_TUNING_VARIANT 15        /* a form only tuning builds launch */

#define RK_GEMM_POLICY_LAUNCH 0          /* the dispatcher as given */
#define RK_GEMM_POLICY_AUTO 1            /* NCF's dX policy: whole-K, or parked K-slices added in slice order + epilogue */
#define RK_GEMM_POLICY_FWD_BLOCKED 2     /* NCF's blocked training forward: 8 k-blocks combined pairwise, + bias, ReLU */

/* One GEMM request, csrc/gemm.h GemmArgs field for field: C[m, n] = epilogue(sum_k A(m, k) * B(n, k)), every sum the chain
 * s = fmaf(a[k], b[k], s), k = 0..K-1.  All pointers are device pointers; strides are in floats. */
typedef struct rk_gemm_desc {
    int32_t M, N, K;
    int32_t policy;                            /* RK_GEMM_POLICY_* */
    const float *A; int64_t a_rs, a_cs;        /* A(m, k) = A[row(m) * a_rs + k * a_cs], row(m) = a_ridx ? a_ridx[m] : m */
    const int32_t *a_ridx;                     /* optional row gather of A (and of row_bias) */
    int32_t a_rmod, a_roff;                    /* a_rmod > 0 (a_ridx == NULL): row(m) = (m + a_roff) % a_rmod */
    const float *acc_init; int32_t ld_init, init_base;   /* optional (needs a_rmod > 0): the chain of C(m, n) starts at
                                                * acc_init[((m + a_roff) / a_rmod - init_base) * ld_init + n] instead of 0 */
    const float *B; int64_t b_rs, b_cs;        /* B(n, k) = B[n * b_rs + k * b_cs] */
    float *C; int32_t ldc, reserved0;
    const float *col_bias;                     /* s + col_bias[n] */
    const float *row_bias;                     /* (with col_bias) ((s + row_bias[row(m)]) + col_bias[n]) + const_add */
    float const_add;
    int32_t relu;                              /* max(s, 0) */
    int32_t sigmoid;                           /* 1 / (1 + expf(-s)) */
    uint32_t drop_thresh24;                    /* > 0: keep element (m, n) iff the counter hash of m * N + n under drop_seed is */
    float drop_scale; int32_t reserved1;       /*      below drop_thresh24 (= keep_prob * 2^24); kept values times drop_scale */
    uint64_t drop_seed;
    const float *mask; int32_t ldmask, reserved2;   /* keep s only where mask[m * ldmask + n] > 0 */
    float *sk_part; int64_t sk_stride;         /* split_k > 1: slice q STORES its partial at sk_part[q * sk_stride + m * ldc + n];
                                                * NULL: every slice ADDS its partial into C (float atomics, order not fixed) */
    int32_t split_k, reserved3;                /* > 1: requested K-slices (no epilogue; 64-tile forms only).  K <= 32 is one
                                                * chunk, hence one slice: it STORES its whole-K result like split_k <= 1 */
    float *scratch; int64_t scratch_floats;    /* policies 1 and 2: the K-slice workspace (rk_ncf_desc.gemm_scratch) */
} rk_gemm_desc;

/* TEST AND DIAGNOSTIC ENTRY: runs one GEMM through the very dispatcher and host policies the NCF tower and the scoring paths
 * use, and reports which kernel took it -- so a test can pin every form against the k-ordered chain at the element.  No
 * product path calls it.  policy 0 hands the request to the dispatcher as given; policy 1 is the tower's dX policy
 * (contiguous C and mask: ldc == ldmask == N; col_bias / relu / mask only; scratch == NULL or N % 4 != 0: whole-K); policy 2
 * is the blocked training forward (A and B k-contiguous and dense, K % 256 == 0, N % 4 == 0, col_bias optional, relu
 * REQUIRED, scratch of >= 8 * 64 * N floats: less makes it fail with RK_EINVAL).
 * form_out (nullable, int32[2]): RK_GEMM_* of the launch and of the right strip's launch (0 where there is none: only
 * RK_GEMM_WIDE_12 hands a strip on).  splits_out (nullable): the K-slices actually used (1 = whole-K).
 * RK_EINVAL, nothing launched: a request the kernels would read or write out of bounds for (missing operand, ldc / ldmask /
 * ld_init < N, row_bias without col_bias, acc_init without a_rmod, an epilogue or a gather together with split_k, parked
 * slices that overlap) or that the policy does not take. */
int rk_gemm_f32(const rk_gemm_desc *desc, int32_t *form_out, int32_t *splits_out, void *stream);

/* ---------------------------------------------------------------- defender --------- */
/* PCASelectUsers (recad/model/defense/PCASelectUsers.py:47-93, registry recad/default.py:223-228) without the dense
 * U x I array and the I x I covariance: C.X = D^-1 A^T (A (D^-1 X)), A the U x I rating CSR, D = diag(sigma_j).
 * All device pointers; asynchronous on `stream` unless stated otherwise.  recad_amd/defense/pca_select_users.py drives
 * them (block subspace iteration with Rayleigh-Ritz replaces scipy.sparse.linalg.eigs, PCASelectUsers.py:66). */

/* A^T as a CSR (n_cols rows, users ascending inside a row): radix sort of (col << 32 | row) keys with the values as
 * payload and stream-ordered temporaries.  Reads rowptr[n_rows] back (synchronous).  Replaces the csr_matrix(dataArray)
 * / np.transpose of PCASelectUsers.py:61-64. */
int rk_pca_transpose(int32_t n_rows, int32_t n_cols, const int32_t *rowptr, const int32_t *col, const float *val,
                     int32_t *t_rowptr /*[n_cols+1]*/, int32_t *t_col /*[nnz]*/, float *t_val /*[nnz]*/, void *stream);
/* sklearn.preprocessing.scale(csr, axis=0, with_mean=False) (PCASelectUsers.py:62): per column the population variance
 * over all n_users rows (zeros included) in fp64, rounded to fp32; var < 10 * FLT_EPSILON -> 1.  inv_scale[j] = 1 / sigma_j;
 * sigma (optional) = sigma_j.  From the rows of A^T (rk_pca_transpose), deterministic. */
int rk_pca_col_scale(int32_t n_cols, int32_t n_users, const int32_t *t_rowptr, const float *t_val, float *inv_scale /*[n_cols]*/,
                     float *sigma /*[n_cols] or NULL*/, void *stream);
/* Y = diag(r_out) . A . diag(c_in) . X for X row-major [n_cols, b], Y [n_rows, b], b in {8, 16}; c_in / r_out may be
 * NULL (no scale).  X and Y 16-byte aligned.  One half of the covariance product covSM = S^T S (PCASelectUsers.py:64-66). */
int rk_pca_spmm(int32_t n_rows, const int32_t *rowptr, const int32_t *col, const float *val, const float *c_in,
                const float *r_out, int32_t b, const float *X, float *Y, void *stream);
/* dist[u] = sum_e val[e]^2 * w[col[e]], w[j] = sum_{c < k} V[j * ldv + c] (w written to `w`, [n_cols]): the distances
 * np.dot(dataArray**2, real(vecs)) summed over the k columns (PCASelectUsers.py:68-78), fp64 accumulation. */
int rk_pca_sq_spmv(int32_t n_rows, int32_t n_cols, const int32_t *rowptr, const int32_t *col, const float *val, const float *V,
                   int32_t ldv, int32_t k, float *w, float *dist /*[n_rows]*/, void *stream);
/* G = Z^T Z, Z = [P | Q] (P [n, p], Q [n, q] row-major, Q may be NULL with q = 0, p + q <= 32), fp64, G [(p+q)^2]
 * row-major.  part: double[RK_PCA_GRAM_BLOCKS * (p+q)^2] scratch.  Fixed reduction order (deterministic). */
#define RK_PCA_GRAM_BLOCKS 256
int rk_pca_gram(int64_t n, const float *P, int32_t p, const float *Q, int32_t q, double *part, double *G, void *stream);
/* out = V . M, V [n, p] fp32, M [p, q] fp64 (device), out [n, q] fp32 (not aliasing V); p, q <= 32. */
int rk_pca_update(int64_t n, const float *V, int32_t p, const double *M, int32_t q, float *out, void *stream);
/* order[0..m) = the ids of the m smallest dist, ties to the lower id: Python's stable sorted(..., key=dist) of
 * PCASelectUsers.py:80 (one 64-bit radix key per user).  Synchronous; RK_EINVAL when a distance is not finite. */
int rk_pca_select(int32_t n, const float *dist, int32_t m, int32_t *order, void *stream);

/* KnnSelectUsers: DegSim, a profile's mean cosine similarity to its k nearest neighbours (Chirita et al. 2005; Burke /
 * Mobasher et al. 2006), exact and repeatable.  It has no counterpart in the reference; the definition is this:
 *   q_e = (int) val_e, every value an integer in 1..127; column ids strictly ascending inside a row, in [0, n_items);
 *   d_uv = sum_i q_ui q_vi in integers; n_u = d_uu < 2^31 (so every d_uv fits int32);
 *   r_u = (float)(1.0 / sqrt((double) n_u)) (IEEE fp64 sqrt and divide, one rounding), 0 for an empty row;
 *   w_uv = ((float) d_uv * r_u) * r_v: round-to-nearest conversion, two fp32 multiplies in that order, no contraction;
 *   candidates of u: every v != u (w = 0 without overlap); k_eff = min(k, U - 1);
 *   topw[u, 0..k) = the k_eff largest w_uv in descending order, padded with 0.0f (values only, never ids);
 *   degsim[u] = (float)(s / k_eff), s the fp64 sum of topw[u, 0..k_eff) in that order; 0 when k_eff == 0 or the row is empty.
 * recad_amd/defense/knn_select_users.py drives these entries.  All pointers are device pointers. */
#define RK_KNN_MAX_K 128
/* Users whose int32 accumulators one workgroup holds at once: 4 * band bytes plus the selection scratch (top list, one
 * 2048-bin digit histogram, hand-over words: 8768 bytes) within the 160 KiB of a CU's LDS. */
#define RK_KNN_MAX_BAND 38720
/* status[0] of rk_knn_norms */
#define RK_KNN_BAD_VALUE 1    /* a value that is not an integer in 1..127 (NaN, 0, 128, 2.5, -1 ...) */
#define RK_KNN_BAD_COLUMN 2   /* column ids of a row not strictly ascending, or outside [0, n_items) */
#define RK_KNN_BAD_NORM 3     /* n_u >= 2^31 */
#define RK_KNN_BAD_ROWPTR 4   /* rowptr[u] negative or above rowptr[u + 1]: the row is not read */
/* Validates the rules above and writes rnorm[u] = r_u.  Synchronous: reads status (device, int32[2]) back.  Without a
 * violation status = {0, -1}.  With one: RK_EINVAL, status = {rule, row} of the lowest offending row (of several rules broken
 * in that row the lowest-numbered one) and rnorm is UNTOUCHED: the values are formed in a temporary and copied on success. */
int rk_knn_norms(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val, float *rnorm /*[U]*/,
                 int32_t *status /*int32[2]*/, void *stream);
/* topw and degsim of every user, from a CSR that passed rk_knn_norms, its rnorm, and its transpose colptr / crow / cval
 * (rk_pca_transpose: users ascending inside a column -- each column is binary-searched for a band's segment).  One
 * workgroup per user; the dots of `band` candidate users at a time are accumulated with integer LDS atomics (exact in any
 * arrival order), turned into w and folded into a running top-k of values by a radix select on their bit patterns.
 * band: 0 = automatic (the users in equal bands of at most 8192), else a multiple of 64 in 64..RK_KNN_MAX_BAND.
 * 1 <= k <= RK_KNN_MAX_K.  order ([U] or NULL): a permutation of the users, workgroup b takes user order[b] (longest work
 * first); results do not depend on it; an entry outside [0, U) is skipped.  topw ([U * k]) may be NULL.  Asynchronous.
 * RK_EINVAL with nothing launched and nothing written: k or band out of range, a missing pointer. */
int rk_knn_degsim(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                  const int32_t *colptr, const int32_t *crow, const float *cval, const float *rnorm, int32_t k, int32_t band,
                  const int32_t *order /*[U] or NULL*/, float *topw /*[U*k] or NULL*/, float *degsim /*[U]*/, void *stream);
/* order_out[0..m) = the ids of the m smallest scores, or of the m largest when largest != 0; ties to the lower id (-0.0
 * and 0.0 are equal).  The radix sort of rk_pca_select.  Synchronous; RK_EINVAL on a non-finite score or m outside 0..n. */
int rk_knn_select(int32_t n, const float *score, int32_t m, int32_t largest, int32_t *order_out, void *stream);

/* CatchSyncSelectUsers: synchronicity and normality of a user's items over a grid of item features (Jiang, Cui, Beutel,
 * Faloutsos, Yang, "CatchSync: Catching Synchronized Behavior in Large Directed Graphs", KDD 2014), integer-exact and
 * repeatable.  It has no counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending); after
 *   validation the values are ignored, every stored entry is an edge;
 *   d_u = the length of row u; deg_i = the length of column i; reach_i = sum over the users u of column i of d_u (the
 *   un-normalised HITS authority after one step from the all-ones hub vector); reach_i <= nnz < 2^31;
 *   bucket(x, s) for an integer x >= 1 and s = grid_bits in 0..3: e = the index of x's leading one bit, m = the s bits directly
 *   below that bit (zero-filled when e < s), bucket = e * 2^s + m: shifts and masks only, no logarithm;
 *   for every rated item (deg_i >= 1): key_i = bucket(deg_i, s) * 65536 + bucket(reach_i, s); the distinct keys in ascending
 *   order are the cells 0 .. M - 1; cell_of[i] = the item's cell, -1 for an unrated item; N_c = the items of cell c;
 *   N = sum N_c, SB = sum N_c^2, all_equal = 1 when every N_c is the same (M <= 1 included), else 0;
 *   M <= RK_CS_MAX_CELLS and I < RK_CS_MAX_ITEMS = 2^26 (so d * N and d^2 stay below 2^53), more is refused;
 *   n_uc = the number of u's items in cell c; pair_num[u] = sum_c n_uc^2 (the ordered pairs of u's items that share a cell, self
 *   pairs included); back_num[u] = sum_c n_uc N_c = the sum over u's items of N_cell(i), both int64; an entry whose cell_of is
 *   -1 or >= M is skipped (no real graph has one; it keeps a caller's table from indexing outside LDS);
 *   scores, each formed in fp64 from those integers with the operations in the written order and no contraction, rounded once
 *   to fp32; d = d_u; a user with d < min_items (min_items >= 2) gets exactly -1.0f, below every eligible score;
 *     sync:      (pair_num - d) / (d * (d - 1)), the share of distinct item pairs inside one cell;
 *     normality: back_num / (d * N);
 *     residual:  sy - s_min, sy = pair_num / (d * d), n = back_num / (d * N), s_b = SB / (N * N),
 *                s_min = (((M * n) * n - 2 * n) + s_b) / (M * s_b - 1), the least sum p_c^2 under sum p_c = 1 and
 *                sum p_c N_c / N = n (the paper's lower limit of synchronicity at a given normality); with all_equal the
 *                denominator is zero in exact arithmetic, that case is decided on the integers and s_min = 1 / M;
 *   flagged: the flag_count(attack_num, U) users of LARGEST score, ties to the lower id (rk_knn_select with largest = 1).
 * Not built: the converged HITS authority as second feature, the paper's per-bin 3-sigma rule, scoring items.
 * recad_amd/defense/catchsync_select_users.py drives these entries.  All pointers are device pointers. */
#define RK_CS_MAX_CELLS 8192
#define RK_CS_MAX_ITEMS (1 << 26)
/* status[0] of rk_cs_cells (the numbering continues RK_MVAE_*) */
#define RK_CS_BAD_FEATURE 17     /* a negative deg_item or reach, or reach 0 at a rated item (bucket needs x >= 1) */
#define RK_CS_TOO_MANY_CELLS 18  /* reported at the lowest item whose cell index would be >= RK_CS_MAX_CELLS */
#define RK_CS_FORM_AUTO 0        /* rows of up to 512 items by one wave, longer ones by the workgroup */
#define RK_CS_FORM_WAVE 1
#define RK_CS_FORM_WORKGROUP 2
#define RK_CS_SCORE_SYNC 0
#define RK_CS_SCORE_NORMALITY 1
#define RK_CS_SCORE_RESIDUAL 2
/* deg_item and reach of every item from the CSR's row pointers and the transpose colptr / crow that rk_pca_transpose writes.
 * One wave per item, integer sums only.  Asynchronous. */
int rk_cs_features(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *colptr, const int32_t *crow,
                   int32_t *deg_item /*[I]*/, int32_t *reach /*[I]*/, void *stream);
/* Keys, their ranking, counts and SB.  cell_count[c] = N_c for c < M and 0 beyond; info = {M, N, SB, all_equal}.  The arrays
 * need not come from a graph.  Synchronous: reads status (device, int32[2]) back.  Without a violation status = {0, -1}.  With
 * one: RK_EINVAL, status = {rule, item} of the lowest offending item (items that break RK_CS_BAD_FEATURE take no part in the
 * ranking) and cell_of / cell_count / info are UNTOUCHED: they are formed in temporaries and copied on success.
 * RK_EINVAL with nothing launched: grid_bits outside 0..3, n_items >= RK_CS_MAX_ITEMS, a missing pointer. */
int rk_cs_cells(int32_t n_items, const int32_t *deg_item, const int32_t *reach, int32_t grid_bits, int32_t *cell_of /*[I]*/,
                int32_t *cell_count /*[RK_CS_MAX_CELLS]*/, int64_t *info /*[4]*/, int32_t *status /*int32[2]*/, void *stream);
/* pair_num and back_num of every user.  The per-user cell histogram is int32 in LDS, filled with integer LDS atomics; per user
 * the row is walked three times (add 1 to each touched cell, read the counts back and sum them, zero the touched cells), so
 * the histogram is cleared in full once per workgroup.  Two forms that give identical words: one wave per user, each of the four
 * waves on its own M-word slice (16 * M bytes of LDS, 128 KiB at M = 8192), a workgroup serving 32 entries of `order`; one
 * 256-thread workgroup per user (4 * M bytes), a workgroup serving 8 entries in turn.  Workgroup g of G takes the entries g,
 * g + G, g + 2 G ...: a descending order spreads its long rows over all workgroups.  form: RK_CS_FORM_*.  order ([U] or
 * NULL) as in rk_knn_degsim: results do not depend on it, an entry outside [0, U) is skipped.  No float, no global atomics.
 * Asynchronous.  RK_EINVAL with nothing launched: M outside 1..RK_CS_MAX_CELLS, form outside 0..2, a missing pointer. */
int rk_cs_user_sums(int32_t n_users, const int32_t *rowptr, const int32_t *col, const int32_t *cell_of, const int32_t *cell_count,
                    int32_t n_cells, int32_t form, const int32_t *order /*[U] or NULL*/, int64_t *pair_num /*[U]*/,
                    int64_t *back_num /*[U]*/, void *stream);
/* score[u] by the formulas above; mode: RK_CS_SCORE_*.  Asynchronous.  RK_EINVAL with nothing launched: mode outside 0..2,
 * min_items < 2, a missing pointer. */
int rk_cs_scores(int32_t n_users, const int32_t *rowptr, const int64_t *pair_num, const int64_t *back_num, const int64_t *info,
                 int32_t mode, int32_t min_items, float *score /*[U]*/, void *stream);

/* FraudarSelectUsers: greedy peeling towards the densest block of the bipartite rating graph (Hooi, Song, Beutel, Shah, Shin,
 * Faloutsos, "FRAUDAR: Bounding Graph Fraud in the Face of Camouflage", KDD 2016), in integers end to end and repeatable.  It
 * has no counterpart in the reference; the definition is this:
 *   graph: users 0..U-1 and items 0..I-1; every stored entry of the rating CSR is one edge, its value is ignored; the nodes are
 *   v in [0, N), N = U + I: user u is node u, item i is node U + i;
 *   weights: deg_i = the stored entries of column i; w_i = wtab[deg_i], wtab a caller's table uint32 [U + 1] with every entry
 *   met in 1..2^24 = RK_FD_WEIGHT_ONE (the Python layer builds it on the host in float64: rint(2^24 / ln(d + log_offset)) for
 *   FRAUDAR's column weight, 2^24 throughout for plain densest-subgraph peeling, Charikar 2000); the degree is the ORIGINAL one,
 *   the weights do not move during the peel;
 *   priority, uint64: pri[u] = the sum of w_i over the user's items that are still alive; pri[U + i] = w_i * (the alive users
 *   who rated i); nnz < 2^29 = RK_FD_MAX_NNZ, so every sum stays below 2^53;
 *   peel: S_0 = all nodes, f_0 = sum_u pri[u]; at step t = 0 .. N - 1 the alive node v of least (pri, node id) is removed -- a
 *   tie goes to the lower id, so a user goes before an item -- order[t] = v, step_of[v] = t, f_{t+1} = f_t - pri[v], and every
 *   alive neighbour of v loses the weight of the item on that edge (a user v: w_i from each of its items; an item v: its own w
 *   from each of its users); a removed node holds pri = 2^64 - 1 and is not charged again; S_t = {v : step_of[v] >= t},
 *   n_t = N - t; f_t is the sum of the alive users' priorities at every t;
 *   best block: t* = the least t in [0, N) that maximises f_t / n_t, compared exactly and strictly (f_a n_b > f_b n_a as a
 *   128-bit product, so the earliest maximum wins); the block is S_t*; f_t* = 0 means an empty matrix and no block.
 *   The greedy guarantee g(S_t*) >= max_S g(S) / 2, g(S) = f(S) / |S|, holds for any positive column weights, so for these.
 * RK_FD_MAX_NODES: the peel keeps one (pri, id) minimum per 64 nodes, per 64 of those and so on in one workgroup's LDS, 16 bytes
 * and one bit per entry; 2^19 nodes are the largest power of two whose 8323 entries fit 160 KiB.  The yelp shape (N = 89 106)
 * runs; a graph of more nodes (config 4) is refused.
 * Not built: rating-weighted edges, flagging items as a workflow step, batch peeling (Bahmani et al. 2012: another result).
 * recad_amd/defense/fraudar_select_users.py drives these entries.  All pointers are device pointers.  nnz = rowptr[U]: the
 * caller passes it so that the entries can refuse and bound on the host; a row or column range is clipped to [0, nnz), an id
 * outside its range is skipped. */
#define RK_FD_MAX_NODES (1 << 19)
#define RK_FD_MAX_NNZ (1LL << 29)
#define RK_FD_WEIGHT_ONE (1u << 24)
#define RK_FD_STEPS_PER_LAUNCH 4096
/* status[0] of rk_fd_init (the numbering continues RK_CS_*) */
#define RK_FD_BAD_WEIGHT 19      /* wtab[d] outside 1..2^24 at a degree d some item has (0 included): status[1] is the lowest such d */
#define RK_FD_BAD_DEGREE 20      /* colptr[i + 1] - colptr[i] outside 0..U: status[1] is the lowest such item; it goes before rule 19 */
/* w_item[i] = wtab[deg_i], the initial priorities and info[3] = f_0 (info[0..2] are left alone).  One pass over the CSR, integer
 * sums only.  Synchronous: reads status (device, int32[2]) back.  Without a violation status = {0, -1}.  With one: RK_EINVAL,
 * status = {rule, index} and nothing else is written.  RK_EINVAL with nothing launched: a missing pointer, U or I negative,
 * U + I outside 1..RK_FD_MAX_NODES, nnz outside 0..2^29 - 1. */
int rk_fd_init(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
               const uint32_t *wtab /*[U+1]*/, uint32_t *w_item /*[I]*/, uint64_t *pri /*[N]*/, int64_t *info /*[4]*/,
               int32_t *status /*int32[2]*/, void *stream);
/* The peel.  pri (in, destroyed: 2^64 - 1 everywhere afterwards) and w_item need not come from rk_fd_init: any uint32 weights
 * and any priorities that are the sums defined above and stay below 2^63 peel exactly; f_0 is summed from pri.  order and
 * step_of ([N]) are the permutation and its inverse; f_trace ([N] or NULL): f_trace[t] = f_t; info = {t*, f_t*, n_t*, f_0}.
 * One 1024-thread workgroup; the chain is issued as ceil(N / steps_per_launch) launches on the stream, every launch rebuilds
 * its LDS hierarchy and f from pri and takes the best block so far from info, so the words do not depend on
 * steps_per_launch.  The column ids of a row (and the rows of a column) must be distinct: the neighbours of one node are
 * updated by plain read-modify-writes.  Asynchronous.  RK_EINVAL with nothing launched: a missing pointer (f_trace may be
 * NULL), U or I negative, U + I outside 1..RK_FD_MAX_NODES, nnz outside 0..2^29 - 1, steps_per_launch < 1. */
int rk_fd_peel_ex(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                  const int32_t *crow, const uint32_t *w_item /*[I]*/, uint64_t *pri /*[N]*/, int32_t *order /*[N]*/,
                  int32_t *step_of /*[N]*/, uint64_t *f_trace /*[N] or NULL*/, int64_t *info /*[4]*/, int32_t steps_per_launch,
                  void *stream);
/* the same with steps_per_launch = RK_FD_STEPS_PER_LAUNCH */
int rk_fd_peel(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
               const int32_t *crow, const uint32_t *w_item, uint64_t *pri, int32_t *order, int32_t *step_of, uint64_t *f_trace,
               int64_t *info, void *stream);

/* ItemKNN victim: item-neighbourhood collaborative filtering (Sarwar et al. 2001; Deshpande and Karypis 2004), exact and
 * repeatable.  It has no counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending);
 *   q = (int) val; d_ij = sum_u q_ui q_uj in integers; n_i = d_ii < 2^31 (so every d_ij fits int32);
 *   r_i = (float)(1.0 / sqrt((double) n_i)), 0 for an item nobody rated (rk_knn_norms applied to the transpose);
 *   w_ij = ((float) d_ij * r_i) * r_j: one conversion, two fp32 multiplies in that order, no contraction (the operations and
 *   order of the KnnSelectUsers definition, applied to columns);
 *   candidates of item i: every j != i with d_ij > 0, ordered by (w_ij descending, j ascending); k_eff = min(k, I - 1);
 *   the first k_eff candidates fill slots t = 0, 1, ... of item i; unused slots hold id -1 and w = +0.0f;
 *   layout, slot-major: nbr_id[t * n_items + i] (int32), nbr_w[t * n_items + i] (float32), t in [0, k): lanes of the scoring
 *   kernel own consecutive items and read slot t of all of them as one coalesced line;
 *   score(u, i) = s_k, s_0 = +0.0f, s_{t+1} = s_t + fl(w_t * (float) q_{u, id_t}): fp32, no contraction, t ascending; a slot
 *   with id -1 or an item u has not rated contributes nothing (the same bits as adding +0.0f: every partial sum is >= 0).
 *   The un-normalised sum of Deshpande and Karypis (2004): no denominator, no shrinkage.  Items u has rated are scored like
 *   any other; excluding them is rk_topk_rows' job.
 * w carries at most five roundings, each term one more and the sum k - 1 more: every score lies within
 * (k + 6) * 2^-24 * sum_t w_t q_t of the float64 evaluation of the same neighbour list.
 * recad_amd/victim/itemknn.py drives these entries.  All pointers are device pointers. */
/* Candidate items whose int32 accumulators one neighbour workgroup holds at once: 4 * band bytes plus the selection scratch
 * (512 64-bit keys: the running list, 256 pending candidates, padding; hand-over words: 4160 bytes) within the 160 KiB of a
 * CU's LDS. */
#define RK_ITEMKNN_MAX_BAND 39872
/* The largest catalogue rk_itemknn_scores takes: one user's row as bytes, one per item, within a CU's LDS (160 KiB less the 64
 * bytes every kernel here leaves free; the kernel needs no other LDS). */
#define RK_ITEMKNN_MAX_ITEMS 163776
#define RK_ITEMKNN_MAX_USER_BLOCK 16
/* The neighbour tables of every item, from a CSR that passed rk_knn_norms, its transpose colptr / crow / cval
 * (rk_pca_transpose) and rnorm_item = the rnorm rk_knn_norms gives for the transpose.  One workgroup per item; the dots of
 * `band` candidate items at a time are accumulated with integer LDS atomics (exact in any arrival order); the candidates become
 * 64-bit keys (bits of w) << 32 | (0xFFFFFFFF - j), all distinct, of which the k_eff largest are kept and sorted.
 * band: 0 = automatic (the items in equal bands of at most 8192), else a multiple of 64 in 64..RK_ITEMKNN_MAX_BAND.
 * 1 <= k <= RK_KNN_MAX_K.  order ([I] or NULL): a permutation of the items, workgroup b takes item order[b]; results do not
 * depend on it; an entry outside [0, I) is skipped.  Every slot of both tables is written.  Asynchronous.
 * RK_EINVAL with nothing launched and nothing written: k or band out of range, a missing pointer.
 * The entry does not care which side of the matrix it is pointed at: called on the transposed roles (the transpose as the CSR,
 * the CSR as the transpose, the users' rnorm) it writes the user-user tables of the UserKNN victim, see below. */
int rk_itemknn_neighbors(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                         const int32_t *colptr, const int32_t *crow, const float *cval, const float *rnorm_item, int32_t k,
                         int32_t band, const int32_t *order /*[I] or NULL*/, int32_t *nbr_id /*[k*I]*/, float *nbr_w /*[k*I]*/,
                         void *stream);
/* out[b * n_items + i] = score(user_ids[b], i) for b in [0, nb), every i: every element of out is written.  A workgroup
 * stages user_block users' rows in LDS as dense byte rows (q <= 127) and walks the items, so each table entry is read once per
 * user block and feeds user_block accumulators, each summed in slot order.  user_block: 0 = automatic (what fits, at most
 * RK_ITEMKNN_MAX_USER_BLOCK), else 1..RK_ITEMKNN_MAX_USER_BLOCK, refused when that many rows of n_items bytes (padded to 16) do
 * not fit.  user_ids ([nb], int32, in [0, U); repeats allowed) are not checked.  Asynchronous; nb = 0 launches nothing.
 * RK_EINVAL with nothing launched and nothing written: k or user_block out of range, n_items > RK_ITEMKNN_MAX_ITEMS, a
 * missing pointer. */
int rk_itemknn_scores(int32_t n_items, int32_t k, const int32_t *nbr_id, const float *nbr_w, const int32_t *rowptr,
                      const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids, int32_t user_block,
                      float *out /*[nb * n_items]*/, void *stream);
/* out[p] = score(users[p], items[p]), p in [0, n): the same sum in the same order, so the same bits as the matrix entry.  A
 * pair whose user or item id is out of range scores 0.0 and reads nothing.  Asynchronous; n = 0 launches nothing. */
int rk_itemknn_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                           const int32_t *rowptr, const int32_t *col, const float *val, const int64_t *users /*[n]*/,
                           const int64_t *items /*[n]*/, int64_t n, float *out /*[n]*/, void *stream);

/* RP3beta victim: the random-walk item-item recommender (P3alpha: Cooper, Lee, Radzik and Siantos 2014; RP3beta: Christoffel,
 * Paudel, Newell and Bernstein 2015; Paudel et al. 2017), exact in any accumulation order and repeatable to the bit.  It has no
 * counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending) and its
 *   transpose colptr / crow / cval (rk_pca_transpose); q_ui = (int) val; r_u = sum_j q_uj as int64; n_i = the number of raters
 *   of item i = colptr[i + 1] - colptr[i]; alpha and beta finite doubles in [0, 4]; 1 <= k <= RK_KNN_MAX_K;
 *   U < RK_RP3_MAX_USERS = 2^23, so that n_i * 2^40 < 2^63;
 *   steps: for a stored entry (u, j), p = (q_uj / r_u)^alpha in double and P_uj = max(1, rint(2^40 * p)) as int64: the
 *   transition probability of the walk's second step as a 40-bit fixed-point integer.  When alpha is exactly 1, p is the IEEE
 *   quotient and pow is not called; when alpha is exactly 0, p = 1; with these two cases P3 at alpha = 1 is reproducible across
 *   math libraries to the bit; otherwise p = pow(q_uj / r_u, alpha);
 *   factors: fa_i = n_i^-alpha and fb_j = n_j^-beta in double, both 0 for an item nobody rated; exponent 1 is the IEEE quotient
 *   1.0 / n, exponent 0 is 1, otherwise pow((double) n, -exponent);
 *   dots: S_ij = sum over the users u with q_ui > 0 of P_uj, in unsigned 64-bit integers, for j != i: the first step of the walk
 *   is binarised (item i moves to each of its n_i raters with probability 1 / n_i), as in the usual implementation;
 *   weight: w_ij = (float)((((double) S_ij * fa_i) * fb_j) * 2^-40): one conversion of S to double (round to nearest), three
 *   double multiplies in that order, one rounding to fp32 with gradual underflow, no contraction;
 *   neighbours of item i: the candidates are every j != i with S_ij > 0, ordered by the 64-bit key
 *   (bits of w) << 32 | (0xFFFFFFFF - j) descending, that is (w descending, j ascending), ItemKNN's key; k_eff = min(k, I - 1);
 *   the first k_eff candidates fill slots t = 0, 1, ... of item i; layout slot-major as for ItemKNN: nbr_id[t * n_items + i]
 *   (int32), nbr_w[t * n_items + i] (float32); unused slots hold -1 and +0.0f; every slot is written;
 *   score(u, j) = the sum of fl(w_ij * (float) q_ui) over the items i that u has rated and whose kept list contains j: fp32,
 *   taken in ascending order of i, starting from +0.0f, no contraction.  Items u has rated are scored like any other; a user
 *   with no items scores +0.0f everywhere.
 * Fixed point because the dots are sums of probabilities: floats added by atomics would depend on arrival order, ordered sums
 * would serialise the workgroup; integers added by 64-bit LDS atomics are exact in any order, so the tables do not depend on
 * `band`, `order` or the schedule.  The quantisation moves a weight by less than 2^-41 / p_min relative, far below the final fp32
 * rounding.
 * Each term carries one rounding more than w, and the sum carries (m - 1) more for m terms: every score lies within
 * (m + c) * 2^-24 * sum of the terms of the float64 evaluation of the same tables (the same kept ids, w before its rounding to
 * fp32), c = 2: m + 1 fp32 roundings in all, and one more unit covers the second-order terms while m <= 4094
 * (tests/_rp3_restate.py counts m per score).
 * Not built: the row normalisation of the kept weights some implementations add, the personalised PageRank form.
 * recad_amd/victim/rp3beta.py drives these entries.  All pointers are device pointers. */
/* Candidate items whose 64-bit accumulators one neighbour workgroup holds at once: 8 * band bytes plus ItemKNN's selection
 * scratch (4160 bytes) within the 160 KiB of a CU's LDS less the 64 bytes every kernel here leaves free.  Also the widest band of
 * rk_rp3_scores (4 bytes a column there). */
#define RK_RP3_MAX_BAND 19904
#define RK_RP3_MAX_USERS 8388608
/* P[e] of every stored entry (int64 [nnz], in CSR order) and r[u] (int64 [U]).  One wave per row, one pass.  Asynchronous.
 * RK_EINVAL with nothing launched and nothing written: alpha outside [0, 4] or not finite, n_users >= RK_RP3_MAX_USERS, a
 * missing pointer. */
int rk_rp3_steps(int32_t n_users, const int32_t *rowptr, const float *val, double alpha, int64_t *P /*[nnz]*/, int64_t *r /*[U]*/,
                 void *stream);
/* fa[i], fb[i] (double [I]) from the transpose's column pointers.  Asynchronous.  RK_EINVAL with nothing launched and nothing
 * written: alpha or beta outside [0, 4] or not finite, a missing pointer. */
int rk_rp3_factors(int32_t n_items, const int32_t *colptr, double alpha, double beta, double *fa /*[I]*/, double *fb /*[I]*/,
                   void *stream);
/* The neighbour tables of every item from the CSR's rowptr / col, P (any table of positive int64 in CSR order whose column sums
 * stay below 2^63), the transpose's colptr / crow, fa and fb.  One workgroup per item; the dots of `band` candidate items at a
 * time sit in LDS as 64-bit integers, added with LDS atomics; selection as in rk_itemknn_neighbors.
 * band: 0 = automatic (the items in equal bands of at most 4096), else a multiple of 64 in 64..RK_RP3_MAX_BAND.  order ([I] or
 * NULL) as in rk_itemknn_neighbors: results do not depend on it, an entry outside [0, I) is skipped.  Every slot of both tables
 * is written.  Asynchronous.  RK_EINVAL with nothing launched and nothing written: k or band out of range,
 * n_users >= RK_RP3_MAX_USERS, a missing pointer. */
int rk_rp3_neighbors(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const int64_t *P /*[nnz]*/,
                     const int32_t *colptr, const int32_t *crow, const double *fa, const double *fb, int32_t k, int32_t band,
                     const int32_t *order /*[I] or NULL*/, int32_t *nbr_id /*[k*I]*/, float *nbr_w /*[k*I]*/, void *stream);
/* out[b * n_items + j] = score(user_ids[b], j) for b in [0, nb), every j: every element of out is written.  One wave per entry
 * of user_ids, with an fp32 row of one band of columns in LDS; the wave walks the user's items in ascending order and the slots
 * of each item's list across its lanes (the ids of one list must be distinct, as the fit leaves them).  A catalogue wider than
 * the band is so many passes; there is no catalogue cap.  band: 0 = automatic (equal bands of at most 8192), else a multiple of
 * 64 in 64..RK_RP3_MAX_BAND.  user_ids ([nb], int32; repeats allowed): an id outside [0, U) scores like a user with no items.
 * Asynchronous; nb = 0 launches nothing.  RK_EINVAL with nothing launched and nothing written: k or band out of range, a missing
 * pointer. */
int rk_rp3_scores(int32_t n_users, int32_t n_items, int32_t k, const int32_t *nbr_id, const float *nbr_w, const int32_t *rowptr,
                  const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids, int32_t band,
                  float *out /*[nb * n_items]*/, void *stream);
/* out[p] = score(users[p], items[p]), p in [0, n): the same sum in the same order, so the same bits as the matrix entry.  A
 * pair whose user or item id is out of range scores 0.0 and reads nothing.  One wave per pair.  Asynchronous; n = 0 launches
 * nothing. */
int rk_rp3_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w, const int32_t *rowptr,
                       const int32_t *col, const float *val, const int64_t *users /*[n]*/, const int64_t *items /*[n]*/, int64_t n,
                       float *out /*[n]*/, void *stream);

/* UserKNN victim: user-neighbourhood collaborative filtering (Resnick et al. 1994; Breese, Heckerman and Kadie 1998; Herlocker
 * et al. 1999), the recommender the average, segment and bandwagon profiles were designed against (Lam and Riedl 2004): the fake
 * users are built to become neighbours of real ones.  Exact and repeatable.  It has no counterpart in the reference; the
 * definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending) and its
 *   transpose colptr / crow / cval (rk_pca_transpose);
 *   q = (int) val; d_uv = sum_i q_ui q_vi in integers; n_u = d_uu < 2^31; r_u = (float)(1.0 / sqrt((double) n_u)), 0 for a user
 *   with no ratings (rk_knn_norms of the matrix itself);
 *   w_uv = ((float) d_uv * r_u) * r_v: one conversion, two fp32 multiplies in that order, no contraction: the operations and
 *   order of the KnnSelectUsers definition, so the kept weights of user u are the topw of rk_knn_degsim, bit for bit;
 *   neighbours of user u: every v != u with d_uv > 0 is a candidate, ordered by (w_uv descending, v ascending);
 *   k_eff = min(k, U - 1); the first k_eff candidates fill slots t = 0, 1, ... of user u; unused slots hold id -1 and w = +0.0f;
 *   layout, slot-major: nbr_id[t * n_users + u] (int32), nbr_w[t * n_users + u] (float32), t in [0, k);
 *   the fit: NO neighbour kernel of its own.  The tables are written by rk_itemknn_neighbors on the transposed roles, called as
 *     rk_itemknn_neighbors(n_users := I, n_items := U, rowptr := colptr, col := crow, val := cval, colptr := rowptr,
 *                          crow := col, cval := val, rnorm_item := rnorm_user, k, band, order, nbr_id, nbr_w, stream):
 *   that entry keeps the k largest (w descending, id ascending) per row of whichever side it is pointed at;
 *   score(u, j), un-normalised: s_0 = +0.0f; for t = 0 .. k - 1 in ascending slot order, with v = id_t(u): if v has rated j,
 *   s <- s + fl(w_t * (float) q_vj): fp32, two roundings per step, never a fused multiply-add.  Skipped: a slot with id -1, an
 *   id outside [0, U) (a caller's own table), a neighbour who has not rated j.  Items u has rated are scored like any other;
 *   excluding them is rk_topk_rows' job.  A user with no neighbours scores +0.0f everywhere;
 *   score(u, j), normalize = 1: the weighted average of Breese et al. (1998) and Herlocker et al. (1999) without mean-centring:
 *   den = the fp32 sum of w_t over the SAME slots (the kept neighbours who rated j) in the same order, plain adds from +0.0f;
 *   the score is s / den by one IEEE fp32 division when den > 0, else +0.0f.  On implicit data (every q = 1) fl(w * 1) = w, so
 *   numerator and denominator are the same bits and every item a kept neighbour has rated scores exactly 1.0f, every other one
 *   +0.0f: the ranking is left to the tie rule of the selection.  That degeneracy belongs to the definition and is not worked
 *   around; normalize is meant for ratings.
 * w carries at most five roundings, each term one more and the sum k - 1 more: every un-normalised score lies within
 * (k + 6) * 2^-24 * sum_t w_t q_t of the float64 evaluation of the same neighbour list (ItemKNN's count).  Normalised: the
 * numerator as before (k + 6 units, relative, every term being >= 0), the denominator five roundings of w and k - 1 adds plus
 * one unit for the second-order terms (k + 5), the quotient one more and one unit for the cross terms of the three: every
 * score with den > 0 lies within (2 k + 13) * 2^-24 of the float64 quotient of the same list, relative.
 * Not built: mean-centring (Resnick's deviation-from-mean prediction), significance weighting and shrinkage of the similarity,
 * case amplification, inverse user frequency.
 * recad_amd/victim/userknn.py drives these entries.  All pointers are device pointers. */
/* The widest band of rk_userknn_scores: with normalize = 1 a column takes 8 bytes of LDS (numerator and denominator), which fit
 * a CU's 160 KiB less the 64 bytes every kernel here leaves free.  The value is RK_RP3_MAX_BAND's, so that one band serves both. */
#define RK_USERKNN_MAX_BAND 19904
/* out[b * n_items + j] = score(user_ids[b], j) for b in [0, nb), every j: every element of out is written.  One wave per entry
 * of user_ids, with an fp32 row of one band of columns in LDS (two rows when normalize = 1).  The wave reads the user's k ids
 * and weights once, walks the slots in ascending order and spreads each neighbour's row over its lanes, 64 entries at a time:
 * the columns of a row are distinct, so lanes never meet inside a slot, and LDS operations of a wave complete in program order,
 * which gives every column its slot order (the same neighbour in two slots is added twice, in order).  A neighbour row longer
 * than 128 entries is binary-searched for the band's segment, a shorter one is strided whole and filtered.  A catalogue wider
 * than the band is so many passes; there is no catalogue cap.  band: 0 = automatic (equal bands of at most 8192), else a
 * multiple of 64 in 64..RK_USERKNN_MAX_BAND.  user_ids ([nb], int32; repeats allowed): an id outside [0, U) scores +0.0f
 * everywhere.  normalize: 0 or 1.  No float atomics.  Asynchronous; nb = 0 launches nothing.  RK_EINVAL with nothing launched
 * and nothing written: k or band out of range, normalize outside {0, 1}, a missing pointer. */
int rk_userknn_scores(int32_t n_users, int32_t n_items, int32_t k, const int32_t *nbr_id /*[k*U]*/, const float *nbr_w /*[k*U]*/,
                      const int32_t *rowptr, const int32_t *col, const float *val, int32_t nb, const int32_t *user_ids,
                      int32_t normalize, int32_t band, float *out /*[nb * n_items]*/, void *stream);
/* out[p] = score(users[p], items[p]), p in [0, n): the same sum in the same order, so the same bits as the matrix entry.  A
 * pair whose user or item id is out of range scores 0.0 and reads nothing.  One thread per pair: the item is looked up in each
 * kept neighbour's ascending row.  Asynchronous; n = 0 launches nothing.  RK_EINVAL with nothing launched: k out of range,
 * normalize outside {0, 1}, a missing pointer. */
int rk_userknn_pair_scores(int32_t n_items, int32_t n_users, int32_t k, const int32_t *nbr_id, const float *nbr_w,
                           const int32_t *rowptr, const int32_t *col, const float *val, const int64_t *users /*[n]*/,
                           const int64_t *items /*[n]*/, int64_t n, int32_t normalize, float *out /*[n]*/, void *stream);

/* EASE victim: the linear item-item autoencoder with a closed-form fit (Steck 2019, "Embarrassingly Shallow Autoencoders for
 * Sparse Data"), repeatable to the bit.  It has no counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending);
 *   q = (int) val; d_ij = sum_u q_ui q_uj in integers; every d_ii < 2^24, so every d_ij (<= sqrt(d_ii d_jj)) is exactly
 *   representable in fp32; a larger d_ii is refused, reported as {RK_EASE_BAD_GRAM, item} the way rk_knn_norms reports;
 *   A_ij = (float) d_ij for i != j, A_ii = (float) d_ii + lambda: one fp32 add, lambda a finite fp32 > 0; A is row-major
 *   [I * I] with 64-bit offsets, symmetric positive definite with smallest eigenvalue >= lambda;
 *   P = A^-1, computed in place on the device in fp32.  This is the only step that is not pinned to the bit: it is pinned by
 *   an error budget.  With A64 the float64 copy of A, P* = inv(A64) and kappa the ratio of A64's extreme eigenvalues,
 *   max|P - P*| <= I * 2^-24 * kappa * max|P*| (the forward bound of a backward-stable inverse with constant 1), and the tests
 *   hold it to 4 x the error of a plain fp32 numpy walk of the same algorithm plus 2^-23 max|P*|
 *   (tests/_ease_restate.py).  Two runs on the same input give the same bits: nothing in the inverse adds floats atomically;
 *   B_ij = -(float)((double) P_ij / (double) P_jj) for i != j, B_jj = +0.0f, row-major [I * I]: the divisor is the diagonal
 *   of the COLUMN (dividing by P_ii gives B transposed);
 *   score(u, j) = s_n, s_0 = +0.0f, s_{e+1} = s_e + fl((float) q_{u, i_e} * B[i_e, j]) over u's stored entries in column
 *   order: fp32, no contraction.  Items u has rated are scored like any other; excluding them is rk_topk_rows' job.  A user
 *   with no entries scores +0.0f everywhere.
 * recad_amd/victim/ease.py drives these entries.  All pointers are device pointers. */
/* The largest catalogue: B is I x I fp32, 4 * 65536^2 bytes = 16 GiB at the limit (the yelp-shaped 34 474 items take 4.75 GB).
 * The inverse runs in B's own storage and its workspace is I * block floats (16 MiB at the limit), so a fit holds one I x I
 * matrix; a workflow that keeps the clean and the poisoned victim holds two, 32 GiB of an MI355X's 288 GB, which leaves the
 * score chunks (chunk * I floats) and the dataset.  The tile grids index 65536 / 64 = 1024 tiles a side. */
#define RK_EASE_MAX_ITEMS 65536
/* The widths of a block step of rk_ease_invert.  A pivot block is inverted inside one workgroup's LDS (64 x 65 floats), and a
 * 64 x 64 tile of the panels and of the trailing update takes its whole k range from two such arrays (33 KiB). */
#define RK_EASE_BLOCK_SMALL 32
#define RK_EASE_BLOCK_LARGE 64
/* status[0] of rk_ease_gram and rk_ease_invert (the numbering continues RK_KNN_BAD_*) */
#define RK_EASE_BAD_GRAM 5    /* d_ii >= 2^24: status[1] is the lowest such item */
#define RK_EASE_NOT_SPD 6     /* a pivot that is not a finite number > 0: status[1] is its index */
/* A ([I * I]) from the CSR and its transpose colptr / crow / cval (rk_pca_transpose), lambda added to the diagonal.  One
 * workgroup per row of A; the dots of 8192 columns at a time are accumulated with integer LDS atomics (exact in any arrival
 * order) and converted once.  Every element of A is written.  Synchronous: the d_ii rule is validated first and status
 * (device, int32[2]) read back.  Without a violation status = {0, -1}.  With one: RK_EINVAL, status = {RK_EASE_BAD_GRAM, item}
 * and A is UNTOUCHED.  RK_EINVAL with nothing launched and nothing written: I < 1 or above RK_EASE_MAX_ITEMS, lambda not
 * finite or <= 0, a missing pointer. */
int rk_ease_gram(int32_t n_users, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *val,
                 const int32_t *colptr, const int32_t *crow, const float *cval, float lambda, float *A /*[I*I]*/,
                 int32_t *status /*int32[2]*/, void *stream);
/* A <- A^-1 in place: a blocked Gauss-Jordan sweep without pivoting (A symmetric positive definite).  Per block K of `block`
 * indices: D = inv(A_KK) inside one workgroup's LDS; A_Kj <- D A_Kj and A_iK <- -A_iK D for i, j outside K, with the old A_iK
 * kept in work; A_ij <- A_ij - (old A_iK) A_Kj, the product summed in k order on the fp32 MFMA and subtracted once.  block: 0 = automatic
 * (RK_EASE_BLOCK_SMALL up to 32 items, else RK_EASE_BLOCK_LARGE), or one of the two.  work: at least I * block floats (block as
 * resolved), never a second I x I.  Synchronous: status (device, int32[2]) is read back, {0, -1} on success.  A pivot that
 * is not a finite number > 0 stops the sweep (every later kernel returns at once; all device loops are bounded by I):
 * RK_EINVAL, status = {RK_EASE_NOT_SPD, pivot index}, and nothing is claimed about A.  RK_EINVAL with nothing launched and
 * nothing written: I < 1 or above RK_EASE_MAX_ITEMS, an unsupported block, too little workspace, a missing pointer. */
int rk_ease_invert(int32_t n_items, float *A /*[I*I]*/, float *work, int64_t work_floats, int32_t block,
                   int32_t *status /*int32[2]*/, void *stream);
/* B from P as defined; B may be P (the diagonal is read out first).  Every element of B is written.  Asynchronous.
 * RK_EINVAL with nothing launched: I out of range, a missing pointer. */
int rk_ease_weights(int32_t n_items, const float *P /*[I*I]*/, float *B /*[I*I]*/, void *stream);
/* out[b * n_items + j] = score(user_ids[b], j) for b in [0, nb), every j: every element of out is written.  One workgroup per
 * user and 256 consecutive items, one item per lane, so each row of B is read as coalesced lines.  user_ids ([nb], int32, in
 * [0, U); repeats and users with empty rows allowed) are not checked.  Asynchronous; nb = 0 launches nothing.
 * RK_EINVAL with nothing launched and nothing written: I out of range, nb < 0, a missing pointer. */
int rk_ease_scores(int32_t n_items, const float *B, const int32_t *rowptr, const int32_t *col, const float *val, int32_t nb,
                   const int32_t *user_ids, float *out /*[nb * n_items]*/, void *stream);
/* out[p] = score(users[p], items[p]), p in [0, n): the same sum in the same order, so the same bits as the matrix entry.  A
 * pair whose user or item id is out of range scores 0.0 and reads nothing.  Asynchronous; n = 0 launches nothing. */
int rk_ease_pair_scores(int32_t n_items, int32_t n_users, const float *B, const int32_t *rowptr, const int32_t *col,
                        const float *val, const int64_t *users /*[n]*/, const int64_t *items /*[n]*/, int64_t n,
                        float *out /*[n]*/, void *stream);

/* iALS victim: weighted matrix factorisation for implicit feedback fitted by alternating least squares (Hu, Koren and
 * Volinsky 2008, "Collaborative Filtering for Implicit Feedback Datasets").  Given the initial item table a fit is a
 * deterministic function of the ratings.  It has no counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms (values integers in 1..127, columns strictly ascending);
 *   q = (int) val; factor count d, 1 <= d <= RK_IALS_MAX_DIM (any integer: the kernels pad to a multiple of 16 internally);
 *   alpha a finite fp32 >= 0, lambda a finite fp32 > 0;
 *   confidence: w_ui = fl(alpha * (float) q_ui), c_ui = fl(1.0f + w_ui); the preference is 1 on stored entries, 0 elsewhere;
 *   Gram matrix: G = Y^T Y + lambda I over ALL rows of the other side's table Y ([n, d] row-major), fp32, exactly symmetric
 *   (the lower triangle is computed and mirrored), summed in an order fixed by (n, d) alone without float atomics: blocks of
 *   RK_IALS_GRAM_ROWS rows are each one k-ordered fmaf chain from +0.0f (the fp32 MFMA), the blocks' partials are added in
 *   block order, lambda is added to the diagonal last.  That is at most n + 1 roundings of a sum of n exact-product terms:
 *   |G_kl - G*_kl| <= (n + 2) * 2^-24 * (sum_i |y_ik y_il| + lambda delta_kl) against float64;
 *   the system of a row u with stored entries e = 0 .. n_u - 1 in column order:
 *     b_u = s_n, s_0 = +0.0f, s_{e+1} = s_e + fl(c_e * y_{i_e}) per component: fp32, no contraction, bit-exact against numpy;
 *     A_u = G + sum_e w_e y_{i_e} y_{i_e}^T, fp32: for k >= l, t_0 = +0.0f, t_{e+1} = fma(fl(w_e * y_ek), y_el, t_e) over the
 *     entries in column order (the fp32 MFMA; the zero padding of the last chunk of RK_IALS_CHUNK entries adds exact zeros),
 *     then (A_u)_kl = fl(G_kl + t_n), mirrored.  The roundings: one per scaled operand, one per fma, one for the add of G; with
 *     gamma_m = m * 2^-24 / (1 - m * 2^-24), T_kl = sum_e |w_e y_ek y_el| in float64 and e_G the budget of G above,
 *     |(A_u)_kl - A*_kl| <= e_G + gamma_{n_u + 1} T_kl + 2^-24 (|A*_kl| + e_G + gamma_{n_u + 1} T_kl), A* in float64 from the
 *     same fp32 tables, w the fp32 value;
 *     x_u = A_u^-1 b_u by a Cholesky factorisation A_u = L L^T (right-looking, one column at a time: l_pp = sqrt(a_pp),
 *     l_ip = a_ip / l_pp, a_ij <- a_ij - fl(l_ip * l_jp)), forward and back substitution column by column
 *     (z_p = b_p / l_pp, b_i <- b_i - fl(l_ip * z_p)), all in fp32 without contraction, inside the workgroup's LDS;
 *     a row with no entries solves G x = 0 and gives +0.0f everywhere;
 *     a pivot (the value under the square root) that is not a finite number > 0 is a refusal, {RK_IALS_NOT_SPD, lowest such
 *     row}: device loops stay bounded by d, and nothing is claimed about that call's output;
 *   one sweep: X <- the rows solved from Y over the CSR, then Y <- the rows solved from the new X over the transpose
 *   (rk_pca_transpose);
 *   objective: J = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2) over all U * I pairs, evaluated in float64
 *   on the device without the dense matrix: per row x_u^T (Y^T Y) x_u + sum_e [c_e (1 - s_e)^2 - s_e^2] + lambda |x_u|^2,
 *   s_e the double dot of the fp32 rows; the per-row doubles are summed in row order by a fixed tree, and lambda |Y|^2 =
 *   lambda * trace(Y^T Y) is added once;
 *   score(u, i) = x_u . y_i through rk_pair_scores / rk_score_topk, with zero biases and mean 0.0.
 * Conditioning.  A_u >= lambda I in exact arithmetic, so a refusal arises only from non-finite tables or from a conditioning
 * that fp32 cannot carry.  The relative error of x_u is about 0.2 * kappa_2(A_u) * 2^-24, kappa ~ 1 + (|Y^T Y| + alpha sum_e q_e
 * |y_e|^2) / lambda: with ratings 1..5 at density 0.15 and d in {16, 32, 64}, (alpha, lambda) = (1, 0.5) stays under kappa 1.5e2
 * (error 9e-6) and (40, 10) under 1.2e3 (2e-4), while (40, 0.5) or lambda = 0.01 at d = 64 with fewer than d rows reaches
 * kappa 1e6, an error of 1e-1 and, once, a negative fp32 pivot.  This is inherent to fp32 ALS; iterative refinement and fp64
 * solves are out of scope.  The hard bound the tests hold x to (tests/_ials_restate.py derives it), beta = sum_e c_e |y_e|:
 * max|x - x*| <= 2 * 2^-24 * kappa_2(A_u) * [d^1.5 (n + n_u + 3 d + 6) max|x*| + (n_u + 1) |beta|_2 / |A_u|_2].
 * recad_amd/victim/ials.py drives these entries.  All pointers are device pointers; no entry adds floats atomically. */
#define RK_IALS_MAX_DIM 128
/* Stored entries of a row staged in LDS at once, and rows of Y in one block of the Gram matrix. */
#define RK_IALS_CHUNK 64
#define RK_IALS_GRAM_ROWS 256
/* status[0] of rk_ials_half_sweep (the numbering continues RK_EASE_*) */
#define RK_IALS_NOT_SPD 7     /* a pivot that is not a finite number > 0: status[1] is the lowest such row */
/* G ([d * d]) = Y^T Y + lambda I as defined.  work: at least ceil(n / RK_IALS_GRAM_ROWS) * dp * dp floats, dp = d rounded up
 * to a multiple of 16 (one partial per block of rows).  Every element of G is written.  Asynchronous.
 * RK_EINVAL with nothing launched and nothing written: n < 1, d outside 1..RK_IALS_MAX_DIM, lambda not finite or <= 0, too
 * little workspace, a missing pointer. */
int rk_ials_gram(int32_t n, int32_t d, const float *Y /*[n*d]*/, float lambda, float *G /*[d*d]*/, float *work, int64_t work_floats,
                 void *stream);
/* GY ([d * d], double) = Y^T Y without lambda, in float64: blocks of max(32, ceil(n / 1024)) rows summed in row order, the
 * blocks' partials in block order, mirrored.  The objective's Gram matrix.  Asynchronous (its scratch is stream-ordered). */
int rk_ials_gram64(int32_t n, int32_t d, const float *Y /*[n*d]*/, double *GY /*[d*d]*/, void *stream);
/* A_out[b] ([d * d], row-major, both triangles) and b_out[b] ([d]) = the system of row row_ids[b], b in [0, nb): the device
 * code of rk_ials_half_sweep up to the factorisation.  row_ids (int32, in range; repeats and empty rows allowed) are not
 * checked.  G: what rk_ials_gram wrote for Y.  Asynchronous; nb = 0 launches nothing.
 * RK_EINVAL with nothing launched and nothing written: n_cols < 1, d or alpha out of range, nb < 0, a missing pointer. */
int rk_ials_system(int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col, const float *val,
                   float alpha, const float *Y /*[n_cols*d]*/, int32_t nb, const int32_t *row_ids, float *A_out /*[nb*d*d]*/,
                   float *b_out /*[nb*d]*/, void *stream);
/* X_out[u] = x_u for every row u of the CSR: one workgroup per row.  The row's entries are staged in LDS RK_IALS_CHUNK at a
 * time (the tail zero-padded to the MFMA's k = 4), the lower-triangle 16 x 16 tiles of sum_e w_e y y^T are accumulated on the
 * fp32 MFMA, shared among the four waves, G is added, and A_u is factorised and solved in LDS (row stride dp + 1).  order
 * ([n_rows] or NULL) as in rk_knn_degsim: workgroup b takes row order[b] (longest rows first); results do not depend on it; an
 * entry outside [0, n_rows) is skipped.  Asynchronous: status (device, int32[2]) reads {0, -1} after a clean sweep and
 * {RK_IALS_NOT_SPD, lowest refused row} otherwise (an unsigned atomic min over the refusing workgroups).
 * RK_EINVAL with nothing launched and nothing written: n_rows or n_cols < 1, d or alpha out of range, a missing pointer. */
int rk_ials_half_sweep(int32_t n_rows, int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col,
                       const float *val, float alpha, const float *Y /*[n_cols*d]*/, const int32_t *order /*[n_rows] or NULL*/,
                       float *X_out /*[n_rows*d]*/, int32_t *status /*int32[2]*/, void *stream);
/* J[0] = the objective as defined; partial[u] = row u's double.  GY: rk_ials_gram64 of Y.  Asynchronous.
 * RK_EINVAL with nothing launched and nothing written: a size < 1, d, alpha or lambda out of range, a missing pointer. */
int rk_ials_objective(int32_t n_rows, int32_t n_cols, int32_t d, const int32_t *rowptr, const int32_t *col, const float *val,
                      float alpha, float lambda, const float *X /*[n_rows*d]*/, const float *Y /*[n_cols*d]*/,
                      const double *GY /*[d*d]*/, double *partial /*[n_rows]*/, double *J /*[1]*/, void *stream);

/* PGA attacker: projected gradient ascent on the fake profiles through a factorisation fitted by alternating least squares (Li,
 * Wang, Singh and Vorobeychik 2016, "Data Poisoning Attacks on Factorization-Based Collaborative Filtering"), here through one
 * sweep of the iALS surrogate above.  It has no counterpart in the reference; the definition is this:
 *   state: R in [0, 1]^{A x I}, the inclusion strengths of the A fake users, the target columns pinned to 1.  The binarised
 *   profile of row f: the n_t targets and the filler_num non-target items of largest R_fj, ties to the lower id, columns
 *   ascending; every entry carries the rating fake_rating (an integer 1..127), so every fake row has n_t + filler_num entries;
 *   surrogate: iALS (rk_ials_gram, rk_ials_half_sweep) on the real rating CSR with the A binarised rows appended, with its own
 *   d, alpha, lambda.  Of the last sweep: Yo the item table the users were solved from, X all user rows (the fake rows last),
 *   Yp the item table solved from X;
 *   loss on Yp and the real rows of X: for target t the eligible users E_t are the real users with no stored entry at t;
 *   s_uj = x_u . y+_j (the fp32 GEMM), the items u has rated excluded from the softmax; L = sum_t (1 / |E_t|) sum_{u in E_t}
 *   [lse_j s_uj - s_ut].  lse and the softmax are worked out in double from the fp32 scores; D_uj = fl32((softmax_uj - [j = t]) /
 *   |E_t|), exactly +0.0f at rated items and in the rows of users outside E_t; the loss terms stay doubles and are summed in a
 *   fixed order.  g = D^T X_real ([I, d]) through the fp32 GEMM per block of users and target, the partial products added in
 *   (target, block) order;
 *   hypergradient through the last sweep, Yo held constant: wbar = fl(alpha * fake_rating), c_fj = 1 + wbar r_fj; under the linear
 *   relaxation that takes an entry (f, j) from absent (r = 0) to present (r = 1) -- its weight wbar r in the systems, (1 + wbar) r
 *   times the other side's row in the right-hand sides --
 *     z_j = B_j^-1 g_j for every item, B_j the matrix rk_ials_half_sweep factorises for item j over the transpose, G from X;
 *     M = sum_j z_j y+_j^T ([d, d], the fp32 GEMM);
 *     h_f = (1 + wbar) sum_{j in f} z_j - (M + M^T) x_f - wbar sum_{j in f} [s+_fj z_j + (x_f . z_j) y+_j],  s+_fj = x_f . y+_j;
 *     v_f = A_f^-1 h_f, A_f the matrix the user side factorises for fake row f, G from Yo;
 *     grad_fj = (1 + wbar - wbar s+_fj)(x_f . z_j) + (1 + wbar - wbar so_fj)(yo_j . v_f),  so_fj = x_f . yo_j, for every f and j:
 *   the exact derivative of L(Yp(X(R), R)) at the binary point.  It differentiates one sweep, not the converged fixed point;
 *   update: with m = max |grad| (not 0): R <- clip(R - fl(lr * fl(grad / m)), 0, 1), one rounding per operation and no
 *   contraction; a result that is not > 0 becomes +0.0f; m = 0 leaves R alone.  Then the targets are set to 1 and the profile
 *   is selected again.
 * recad_amd/attack/pga.py sequences these entries, rk_gemm_f32 and rk_pca_transpose.  All pointers are device pointers, every
 * entry is asynchronous, none adds floats atomically, and two runs give the same bits. */
#define RK_PGA_MAX_TARGETS 64
/* rk_ials_half_sweep with the right-hand side of row u read from rhs[u * d ..] instead of b_u: A_u is built and factorised by
 * the same device code (so to the same bits), order and status as there.
 * RK_EINVAL with nothing launched and nothing written: n_rows or n_cols < 1, d or alpha out of range, a missing pointer. */
int rk_ials_solve_rhs(int32_t n_rows, int32_t n_cols, int32_t d, const float *G, const int32_t *rowptr, const int32_t *col,
                      const float *val, float alpha, const float *Y /*[n_cols*d]*/, const float *rhs /*[n_rows*d]*/,
                      const int32_t *order /*[n_rows] or NULL*/, float *X_out /*[n_rows*d]*/, int32_t *status /*int32[2]*/,
                      void *stream);
/* A block of nb score rows, row b belonging to user user0 + b of the rating CSR: scores [nb * n_items] holds s_uj on entry and
 * D_uj on return, terms[b] = (lse - s_ut) * inv_count in double (0.0 for a user with eligible[user] == 0, whose row of D is
 * +0.0f).  One wave per row; the sums run lane-strided and then over the wave's butterfly: a fixed order.
 * RK_EINVAL with nothing launched and nothing written: nb or n_items < 1, user0 < 0, a target outside [0, n_items), inv_count
 * not a finite positive number, a missing pointer. */
int rk_pga_loss(int32_t nb, int32_t n_items, float *scores /*[nb*n_items]*/, const int32_t *rowptr, const int32_t *col,
                int32_t user0, int32_t target, const int32_t *eligible /*[n_users]*/, double inv_count, double *terms /*[nb]*/,
                void *stream);
/* out[0] = the sum of n doubles: thread t of one workgroup adds terms t, t + 256, ... in order, then the fixed tree. */
int rk_pga_loss_sum(int64_t n, const double *terms, double *out /*[1]*/, void *stream);
/* out[i] = ((parts[0][i] + parts[1][i]) + parts[2][i]) + ...: n_parts arrays of n floats added in order. */
int rk_pga_add_blocks(int64_t n, int32_t n_parts, const float *parts /*[n_parts*n]*/, float *out /*[n]*/, void *stream);
/* H[f] = h_f for the n_fake rows of the fake CSR (fptr, fcol): one workgroup per row.  s+ and q = x . z are d-long fmaf chains
 * over the lanes and the wave's butterfly.  (1 + wbar) z_j - wbar s+ z_j cancels to one part in wbar on a fitted entry (s+ near
 * 1), so the coefficient cf = fl(1 + fl(wbar fl(1 - s+))) is formed first; the sparse sum runs in column order,
 * t += fl(fl(cf z_j) - fl(fl(wbar q) y+_j)), and h = fl(t - m), m the l-ordered sum of fl(fl(M_kl + M_lk) x_l), no contraction.
 * RK_EINVAL with nothing launched and nothing written: a size < 1, d or wbar out of range, a missing pointer. */
int rk_pga_user_adjoint(int32_t n_fake, int32_t n_items, int32_t d, const float *Z /*[I*d]*/, const float *Yp /*[I*d]*/,
                        const float *Xf /*[A*d]*/, const float *M /*[d*d]*/, const int32_t *fptr /*[A+1]*/, const int32_t *fcol,
                        float wbar, float *H /*[A*d]*/, void *stream);
/* grad [A * I] as defined: four k-ordered fmaf chains of length d per element (x.z, x.y+, x.yo, yo.v), combined as
 * (1 + wbar (1 - s+)) (x.z) + (1 + wbar (1 - so)) (yo.v) (the coefficients as in rk_pga_user_adjoint); eight fake rows held in
 * LDS across a tile of 256 items.  gmax[0] = the bit pattern of max |grad| (an integer max: order-free), 0 for a zero gradient.
 * RK_EINVAL with nothing launched and nothing written: a size < 1, d or wbar out of range, a missing pointer. */
int rk_pga_grad(int32_t n_fake, int32_t n_items, int32_t d, const float *Xf, const float *V, const float *Z, const float *Yp,
                const float *Yo, float wbar, float *grad /*[A*I]*/, uint32_t *gmax /*[1]*/, void *stream);
/* The update (grad == NULL or gmax[0] == 0: none), the pinning of the targets and the selection, one workgroup per row of any
 * length: a radix select over the bit patterns finds the filler_num-th largest non-target strength, an ordered compaction writes
 * the n_targets + filler_num columns of row f ascending at fcol_out[f * (n_targets + filler_num) ..].  targets: distinct ids in
 * [0, n_items) (the caller checks them).
 * RK_EINVAL with nothing launched and nothing written: a size < 1, n_targets outside 1..RK_PGA_MAX_TARGETS, filler_num outside
 * [0, n_items - n_targets], lr not a finite positive number (with grad), a missing pointer. */
int rk_pga_step(int32_t n_fake, int32_t n_items, float *R /*[A*I]*/, const float *grad /*[A*I] or NULL*/, const uint32_t *gmax,
                float lr, int32_t n_targets, const int32_t *targets, int32_t filler_num, int32_t *fcol_out, void *stream);

/* SLIM victim: sparse linear item-item weights (Ning and Karypis 2011, "SLIM: Sparse Linear Methods for Top-N Recommender
 * Systems"): each item's column is an elastic-net regression on the other items with non-negative weights and a zero diagonal,
 * fitted by cyclic coordinate descent and repeatable to the bit.  It has no counterpart in the reference; the definition is this:
 *   input: the U x I rating CSR under the rules of rk_knn_norms and the d_ii rule of rk_ease_gram;
 *   G = what rk_ease_gram(..., lambda = beta, ...) writes: G_ik = (float) d_ik off the diagonal, an exact integer, and
 *   G_kk = fl((float) d_kk + beta), beta a finite fp32 > 0; row-major [I * I] with 64-bit offsets;
 *   l1 a finite fp32 >= 0, sweeps an integer >= 1;
 *   all arithmetic is fp32, every operation rounded on its own, no contraction (IEEE with gradual underflow);
 *   column j: w_k = +0.0f for every k and r_i = G[i * I + j] for every i (the diagonal entry is included, but never read as a
 *   coordinate); for s = 1 .. sweeps, for k = 0 .. I - 1 ascending except k = j, one coordinate step:
 *     t = fl(r_k - l1); q = fl(t / G_kk), a correctly rounded division; v = fl(w_k + q); w' = v > 0 ? v : +0.0f;
 *     delta = fl(w' - w_k); when delta == 0 nothing happens; otherwise w_k = w' and r_i = fl(r_i - fl(delta * G[k * I + i])) for
 *     every i in [0, I), i = k and i = j included: ROW k of G is the one read;
 *   a coordinate with w_k == +0 and r_k <= l1 always gives delta == 0 and may be passed over without dividing; a sweep that
 *   changes no coordinate leaves the state as it is for every later sweep, so a column stops there;
 *   W[k * I + j] = w_k, W[j * I + j] = +0.0f: W is oriented like EASE's B, and score(u, j) is rk_ease_scores /
 *   rk_ease_pair_scores on W unchanged;
 *   info[3 * j + 0] = the index (from 1) of the last sweep that changed a coordinate of column j, 0 when none did,
 *   info[3 * j + 1] = the number of w_k > 0, info[3 * j + 2] = the number of steps with delta != 0;
 *   R_out[i * I + j] = r_i after the last sweep.
 * Each column minimises f_j(w) = 1/2 w^T G w - d_j^T w + l1 sum_k w_k over w >= 0, w_j = 0: the L2 weight is beta / 2 on |w|^2.
 * recad_amd/victim/slim.py drives the entry.  All pointers are device pointers. */
/* The largest catalogue.  One workgroup owns a column and keeps r and w in LDS, 8 * I bytes, beside 64 bytes in which its four
 * waves agree on the next coordinate.  A gfx950 workgroup may take 160 KiB = 163 840 bytes, of which the library's launches
 * leave 64 unused: (163 840 - 64 - 64) / 8 = 20 464 items.  A fit holds two I x I fp32 matrices, G (a temporary) and W:
 * 2 * 4 * 20 464^2 bytes = 3.35 GB at the limit.  The yelp-shaped catalogue (34 474 items) is out of reach: it is refused. */
#define RK_SLIM_MAX_ITEMS 20464
/* status[0] of rk_slim_fit (the numbering continues RK_IALS_*) */
#define RK_SLIM_BAD_DIAG 8    /* a G_kk that is not a finite number > 0: status[1] is the lowest such k */
/* W ([I * I]) from G as defined; info ([3 * I]) and R_out ([I * I]) may each be NULL.  One workgroup per column: 256
 * coordinates at a time are worked out from the current r, the lowest one whose step is not zero is applied (row k of G read
 * as coalesced lines, the update of r spread over the workgroup), and the coordinates after it are worked out again.  Every
 * element of W, info and R_out is written.  All device loops are bounded by I and sweeps; nothing adds floats atomically.
 * The diagonal is validated first and status (device, int32[2]) read back, which is the call's only synchronisation: {0, -1}
 * without a violation; with one RK_EINVAL, status = {RK_SLIM_BAD_DIAG, lowest index} and W, info and R_out are UNTOUCHED.
 * RK_EINVAL with nothing launched and nothing written: I < 1 or above RK_SLIM_MAX_ITEMS, sweeps < 1, l1 negative or not
 * finite, G, W or status missing. */
int rk_slim_fit(int32_t n_items, const float *G /*[I*I]*/, float l1, int32_t sweeps, float *W /*[I*I]*/,
                int32_t *info /*[3*I] or NULL*/, float *R_out /*[I*I] or NULL*/, int32_t *status /*int32[2]*/, void *stream);

/* ---------------------------------------------------------------- APR victim --------- */
/* Adversarial Personalized Ranking (He, He, Du and Chua, SIGIR 2018, "Adversarial Personalized Ranking for Recommendation"):
 * matrix factorisation under the BPR loss with a second BPR term evaluated at the embeddings moved by the worst-case
 * perturbation of size eps.  With adv_reg = 0 it is plain BPR-MF.  It has no counterpart in the reference; the definition is this:
 *   tables: P [U, d] and Q [I, d], fp32, ONE [N = U + I, d] allocation, users first; item i is row U + i;
 *   a step is a minibatch of B triplets (u_b, i_b, j_b) = (user, positive, negative), the sign convention of rk_bpr_rows;
 *   1. data term: x_b = <p_u, q_j> - <p_u, q_i>; c_b = sigma(x_b) / B; L = (1 / B) sum_b softplus(x_b);
 *      R = (lambda / 2B) sum_b (|p_u|^2 + |q_i|^2 + |q_j|^2);
 *   2. Gamma, the gradient of L alone (not of R): row r sums its incidences in ascending order of 3 b + role (role 0 = user,
 *      1 = positive, 2 = negative): Gamma_P[u] = sum c_b (q_j - q_i); Gamma_Q[i] = sum_{b: i_b = i} (-c_b p_u) +
 *      sum_{b: j_b = i} (c_b p_u).  An item that is positive in some triplets and negative in others has ONE row;
 *   3. perturbation, per row: n_r = sqrt(sum_k Gamma_rk^2); s_r = eps / max(n_r, 1e-12f), and s_r = 0 when n_r == 0;
 *      Delta_rk = Gamma_rk * s_r.  A row whose Gamma is all zero gets exact zeros, whatever eps is.  Delta is a constant of the step: nothing is differentiated through it;
 *   4. adversarial term: p' = p_u + Delta_P[u], q'_i = q_i + Delta_Q[i], q'_j = q_j + Delta_Q[j];
 *      x'_b = <p', q'_j> - <p', q'_i>; c'_b = sigma(x'_b) / B; L' = (1 / B) sum_b softplus(x'_b);
 *   5. the gradient of L + adv_reg L' + R: row r adds, per incidence and in the same order, (a) the term of step 2, (b) adv_reg
 *      times the same term formed from c' and the moved partner rows, (c) (lambda / B) * its own row;
 *   6. update: dense torch.optim.Adam over all N rows (untouched rows have g = 0 and their moments still decay), the
 *      arithmetic of rk_adam_step.
 *   Rounding: in steps 2 and 5 every product and every addition is fp32 and rounded on its own, in the written order, from
 *   +0.0f: a term is fl(c * fl(q_j - q_i)), fl((-c) * p_u) or fl(c * p_u); the moved rows are fl(q + Delta); (b) is
 *   fl(adv_reg * term'); (c) is fl(fl(lambda / (float) B) * self).  The dots, sigma(x) / B, softplus and the loss sums are worked out in double from the
 *   fp32 rows and rounded once: x and c are the fp32 values nearest to them; the norms use a fixed fp32 tree.  Nothing adds
 *   floats atomically: the same call gives the same bits.
 *   Switches: with adv_reg == 0 steps 2-4 are not run (their workspace areas are not written, (b) is not added, L' = 0); with
 *   eps == 0, Delta = 0 and L' = L.
 * B is `batch` for every step but the last, which has n - (n_steps - 1) * batch triplets and divides by that.
 * recad_amd/victim/apr.py drives the entries.  All pointers but the layout and the descriptor are device pointers. */
#define RK_APR_MAX_DIM 256
#define RK_APR_MAX_BATCH 65536
/* status[0] of rk_apr_train_epoch (the numbering continues RK_SLIM_*); status[1] is the lowest offending triplet */
#define RK_APR_BAD_USER 9     /* users[t] outside [0, n_users) */
#define RK_APR_BAD_POS 10     /* pos[t] outside [0, n_items) */
#define RK_APR_BAD_NEG 11     /* neg[t] outside [0, n_items) */
/* Byte offsets of the workspace's areas (each a multiple of 256, and 256 bytes that nothing writes follow every area).  nb = min(batch, n) is the longest step, T = 3 * nb the most
 * rows a step can touch.  Areas of ONE step, overwritten by the next: x, c, x_adv, c_adv (float [nb]); slot_of (int32 [T]:
 * the slot of the row of incidence 3 b + role); gamma, delta (float [T * dim], row `slot`); norm (float [T]); part (double
 * [3 * part_blocks]: the workgroups' partial sums of softplus(x), of the squared norms and of softplus(x')).  Areas of the
 * epoch: keys (uint64 [3 n], the sorted plan: step << 44 | row << 20 | 3 b + role; step s owns [3 s batch, 3 s batch + 3 nb_s)),
 * keys_in and sort_tmp (the sort's input and scratch), run (int32 [n_steps * run_stride]: per step {n_runs, start_0 ..
 * start_{n_runs}}: slot k is the run of sorted positions [start_k, start_{k+1}) of its step, start_{n_runs} = 3 nb_s),
 * grad (float [N * dim]: the dense gradient of the step, all zero between steps). */
typedef struct rk_apr_layout {
    int64_t bytes;
    int64_t keys, keys_in, sort_tmp, sort_tmp_bytes, run, x, c, slot_of, gamma, norm, delta, x_adv, c_adv, part, grad;
    int32_t run_stride, part_blocks, max_rows, n_steps;
} rk_apr_layout;
typedef struct rk_apr_desc {
    int32_t n_users, n_items, dim, reserved0;
    float *table;             /* [N * dim], users first */
    float *m, *v;             /* Adam moments [N * dim] */
    float *grad;              /* [N * dim] or NULL: receives the dense gradient of the LAST step */
    float lam, eps, adv_reg, lr, beta1, beta2, adam_eps;
    int32_t reserved1;
    void *workspace;
    int64_t workspace_bytes;
} rk_apr_desc;
/* *out = the layout for an epoch of n triplets in steps of `batch`.  Host only, nothing launched.  RK_EINVAL: a size < 1, dim
 * above RK_APR_MAX_DIM, batch above RK_APR_MAX_BATCH, 2^20 steps or more, 2^24 rows or more, n of 2^31 / 3 or more, no `out`. */
int rk_apr_workspace(int32_t n_users, int32_t n_items, int32_t dim, int64_t n, int32_t batch, rk_apr_layout *out);
/* One epoch: ceil(n / batch) steps as defined, Adam steps adam_t0 + 1 ...  The ids are validated first by a kernel that reads
 * nothing else, and status (device, int32[2]) is read back, which is the call's only synchronisation: {0, -1} without a
 * violation; with one RK_EINVAL, status = {RK_APR_BAD_*, lowest such triplet} and nothing else is launched or written.  Then
 * the plan (keys, one radix sort, the run table) once, and per step five launches: apr_coef_kernel<VEC4, ADV = 0> (x, c, partial sums),
 * apr_rows_kernel<GRAD = 0, REGS> (one wave per touched row: Gamma, n, Delta, slot_of), apr_coef_kernel<VEC4, ADV = 1> (x', c'),
 * apr_rows_kernel<GRAD = 1, REGS> (one wave per touched row: the row of step 5 into the dense gradient) and apr_adam_kernel,
 * the Adam pass over all N * dim elements, which stores 0
 * in place of every gradient it reads, copies it to desc->grad when that is given, updates only with apply_update != 0, and
 * writes losses[3 s .. 3 s + 2] = {L, L', R} of step s (device, double, summed in a fixed order).
 * RK_EINVAL with nothing launched and nothing written: dim outside 1..RK_APR_MAX_DIM, batch outside 1..RK_APR_MAX_BATCH,
 * n <= 0, eps or adv_reg negative or not finite, adam_t0 < 0, a workspace smaller than rk_apr_workspace says or not
 * aligned to 256 bytes, a missing pointer, apply_update == 0 without desc->grad, the limits of rk_apr_workspace. */
int rk_apr_train_epoch(const rk_apr_desc *desc, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t n,
                       int32_t batch, int32_t adam_t0, int32_t apply_update, double *losses /*[3*n_steps]*/,
                       int32_t *status /*int32[2]*/, void *stream);
/* One epoch of n_rep independent APR models ("members") in shared launches.  Definition: for every member r, table, m, v, desc.grad
 * when given, losses[r] and status[2 r .. 2 r + 1] hold, bit for bit, what
 *   rk_apr_train_epoch(&descs[r], users[r], pos[r], neg[r], n[r], batch, adam_t0[r], apply_update, losses[r], status + 2 r, stream)
 * leaves on copies of the same inputs (the APR definition above), and so do the areas of the member's workspace.  Members may
 * differ in n_users, n_items, n (so in their step counts), lam, eps, adv_reg, lr, the betas, adam_eps and adam_t0; each has its own
 * workspace, sized by rk_apr_workspace; dim, batch and apply_update are common.  descs, n, adam_t0 and the four pointer arrays are
 * HOST arrays of n_rep entries; what users[r], pos[r], neg[r] and losses[r] (double [3 * n_steps_r]) point to is on the device,
 * as is status (int32 [2 * n_rep]).
 * Launches: the ids of all members are validated by one launch and all status words are read back in one synchronisation, the
 * only one of the call; with a bad id in any member RK_EINVAL, status of member r = {RK_APR_BAD_*, lowest such triplet} or
 * {0, -1} for a clean member, and nothing else is launched or written for any member.  Then the plan of every member (keys, radix
 * sort, run table: one set of launches per member, once per epoch), and for st = 0 .. max_r n_steps_r - 1 ONE launch of each kind
 * for the whole group, the member being the grid's second dimension: the coefficient kernel; the Gamma rows kernel and the
 * adversarial coefficient kernel when at least one member has adv_reg != 0; the gradient rows kernel; the Adam pass.  A workgroup
 * leaves at once when st >= n_steps_r (the member's epoch is over: its tables, moments and zeroed gradient are not touched
 * again), when it lies beyond the member's own grid for this step, or when the kernel is an adversarial one and the member has
 * adv_reg == 0 (its areas of steps 2-4 stay unwritten).  The members' constants (pointers, sizes, hyperparameters, fl(lam / nb) of
 * the full and of the short step) and the Adam coefficients of every (member, step), from the host function rk_apr_train_epoch
 * uses, go to the device once per epoch; a step passes its index alone.  Every member runs the code path rk_apr_train_epoch would
 * take for it (the float4 loads at dim == 64 by its own table's alignment).  No float atomics, no cooperative launch.
 * RK_EINVAL with nothing launched and nothing written: n_rep outside 1..RK_APR_MAX_GROUP, a missing array or pointer, members
 * whose dim differ, anything rk_apr_train_epoch refuses for any member, two members whose table, m, v, grad or workspace byte
 * ranges overlap. */
#define RK_APR_MAX_GROUP 64
int rk_apr_train_epoch_group(int32_t n_rep, const rk_apr_desc *descs, const int64_t *const *users, const int64_t *const *pos,
                             const int64_t *const *neg, const int64_t *n, int32_t batch, const int32_t *adam_t0,
                             int32_t apply_update, double *const *losses, int32_t *status /*int32[2*n_rep]*/, void *stream);

/* ---------------------------------------------------------------- Mult-VAE victim --------- */
/* Mult-VAE (Liang, Krishnan, Hoffman and Jebara, WWW 2018, "Variational Autoencoders for Collaborative Filtering"): a
 * variational autoencoder over a user's row of the implicit matrix with a multinomial likelihood over the whole catalogue and
 * an annealed KL term.  It has no per-user parameters and no counterpart in the reference; the definition is this:
 *   parameters, fp32, in ONE flat buffer in this order (rk_mvae_layout gives the element offsets), so that Adam is one launch:
 *     W1 [I, H] (one row per item: the sparse layer gathers rows), b1 [H]; W2 [2L, H], b2 [2L]; W3 [H, L], b3 [H];
 *     W4 [I, H], b4 [I].  Apart from W1 every weight is stored out x in: the forward products read both operands k-contiguous.
 *   chain(x, W)[u, j] means s = 0; s = fmaf(x[u, k], W[j, k], s) for k ascending: what the whole-K fp32 MFMA GEMM computes, to
 *   the bit; a bias is added afterwards by one fp32 add.
 *   A step works on B users (batch positions 0 .. B - 1, ids may repeat) each with n_u >= 1 stored entries; x_ui = 1 for a
 *   stored entry whatever its value.  `step` is the count of updates so far (step0 + the step's index in the epoch).
 *   1. input: s_u = n_u^-1/2; with S = rk_drop_step_seed of (seed, step) and S_u = rk_drop_step_seed of (S, u), entry (u, i) is
 *      kept iff rk_drop_keep says so for (S_u, i, thresh24) (csrc/common.h), thresh24 = (unsigned)((1 - dropout) * 2^24) with 1 - dropout formed in double from the fp32 dropout;
 *      c_u = s_u / (1 - dropout), in double (1 / sqrt(n_u), then the division), rounded once.  dropout = 0 keeps every entry;
 *   2. sparse layer: a_uh = sum of W1[i, h] over the kept items of row u in ascending item order, fp32 adds from +0.0;
 *      pre1 = fl(fl(c_u * a_uh) + b1[h]); h1 = tanh(pre1) evaluated in double, rounded once;
 *   3. encoder head: ml = chain(h1, W2) + b2, [B, 2L]; mu = ml[:, :L], logvar = ml[:, L:];
 *   4. sample: with E = rk_drop_step_seed of (seed ^ 0xA5A5A5A5A5A5A5A5, step), E_u = rk_drop_step_seed of (E, u) and
 *      r_t = rk_mix64 of (E_u ^ t * 0xD1342543DE82EF95) (64-bit wrap), u1 = ((r_{2j} >> 11) + 1) * 2^-53, u2 = (r_{2j+1} >> 11) * 2^-53,
 *      eps[u, j] = sqrt(-2 ln u1) * cos(2 pi u2) in double, rounded once; z = mu + eps * exp(logvar / 2) in double from the
 *      fp32 mu, eps and logvar, rounded once; KL_u = -1/2 sum_j (1 + logvar - mu^2 - exp(logvar)) in double;
 *   5. decoder: pre2 = chain(z, W3) + b3; h2 = tanh(pre2) as in 2; logits = chain(h2, W4) + b4, [B, I];
 *   6. loss, one pass per logits row and in place: lse_u = max + ln(sum_i exp(l_ui - max)) in double; nll_u = sum over ALL the
 *      row's stored items (dropout is on the input only) of (lse_u - l_ui); loss = (1 / B) sum_u (nll_u + beta KL_u), reported
 *      with (1 / B) sum nll and (1 / B) sum KL; dl[u, i] = ((n_u exp(l_ui - lse_u) - x_ui) / B) in double, rounded once,
 *      written over the logits; beta = min(anneal_cap, step / total_anneal_steps) in double (anneal_cap when total_anneal_steps
 *      is 0).  B is the number of rows of this step: a short last step divides by its own size;
 *   7. backward, every product a chain over the summed index in ascending order: gW4 = chain_u(dl, h2); gb4 = the column sums
 *      of dl by fp32 adds in ascending batch position (so are gb3 of dp2, gb2 of dml, gb1 of dp1); dh2 = chain_i(dl, W4);
 *      dp2 = fl(dh2 * fl(1 - fl(h2 * h2))); gW3 = chain_u(dp2, z); dz = chain_h(dp2, W3); dmu = dz + (beta / B) mu and
 *      dlogvar = 1/2 dz eps exp(logvar / 2) + (beta / 2B) (exp(logvar) - 1), each in double and rounded once, dml = [dmu |
 *      dlogvar]; gW2 = chain_u(dml, h1); dh1 = chain_j(dml, W2); dp1 as dp2; gW1[i, h]: acc = +0.0, then acc = fmaf(c_u,
 *      dp1[u, h], acc) over the batch positions that hold i as a KEPT entry, ascending; an item without one gets +0.0;
 *   8. update: torch.optim.Adam over the flat buffer, the arithmetic of rk_adam_step, Adam step number step + 1.
 *   The sums of exp, nll and KL run in fixed trees (tests hold them to rounding budgets); nothing adds floats atomically and
 *   the item-grouped view of the kept entries is built once per step by one radix sort of (item << 12 | batch position): the
 *   same call gives the same bits.
 *   Inference: no dropout (c_u = s_u, and 0 for a user without entries), z = mu, and only the first L rows of W2 are multiplied.
 *   Every product is whole-K at every catalogue size (DESIGN 16 records the price at the largest shape).
 * recad_amd/victim/multvae.py drives the entries.  All pointers but the layout and the descriptor are device pointers. */
#define RK_MVAE_MAX_HIDDEN 1024
#define RK_MVAE_MAX_LATENT 512
#define RK_MVAE_MAX_BATCH 4096
#define RK_MVAE_MAX_ITEMS 262144  /* the row kernel's LDS bitmap: 32 KiB; batch * n_items stays below 2^31 */
/* status[0] of the rk_mvae_* entries (the numbering continues RK_APR_*); status[1] is the lowest offending position */
#define RK_MVAE_BAD_USER 12   /* user_ids[t] outside [0, n_users) */
#define RK_MVAE_BAD_ROW 13    /* the row of user_ids[t] is not strictly ascending inside [0, n_items) */
#define RK_MVAE_EMPTY_ROW 14  /* user_ids[t] has no stored entry (training only) */
#define RK_MVAE_NNZ_CAP 15    /* step status[1] holds more entries than the workspace's nnz_cap */
#define RK_MVAE_BAD_ITEM 16   /* item_ids[t] outside [0, n_items) (rk_mvae_pair_scores) */
/* Byte offsets of the workspace's areas (each a multiple of 256, and 256 bytes that nothing writes follow every area), all of
 * ONE step and overwritten by the next; B = batch, E = nnz_cap, the most stored entries a step may hold.  brp (int32 [B + 1]:
 * prefix sums of the rows' lengths); keep (int32 [E]: entry brp[b] + k is the k-th stored item of batch row b, 1 = kept); keys_in,
 * keys (the sort's input and output; its scratch is allocated on the stream); t_ptr (int32 [I + 1]) and t_row (int32 [E]): item i's kept batch
 * positions are t_row[t_ptr[i] .. t_ptr[i + 1]), ascending; c (float [B]); a, pre1, h1, pre2, h2, dh2, dp2, dh1, dp1 (float
 * [B * H]); ml, dml (float [B * 2L]); eps, z, dz (float [B * L]); kl, lse, nll (double [B]); logits (float [B * I], holds dl
 * after the step); grad (float [n_params], the flat gradient in the parameters' order).  w1 .. b4 and n_params are ELEMENT
 * offsets into the flat parameter buffer, not workspace areas. */
typedef struct rk_mvae_layout {
    int64_t bytes;
    int64_t brp, keep, keys, keys_in, t_ptr, t_row, c, a, pre1, h1, ml, eps, z, kl, pre2, h2, logits, lse, nll,
        dh2, dp2, dz, dml, dh1, dp1, grad;
    int64_t w1, b1, w2, b2, w3, b3, w4, b4, n_params;
    int64_t nnz_cap;
    int32_t batch, reserved;
} rk_mvae_layout;
typedef struct rk_mvae_desc {
    int32_t n_users, n_items, hidden, latent;
    const int32_t *rowptr, *col;   /* the rating CSR, [n_users + 1] and [nnz]; values are not read */
    float *params, *m, *v;         /* the flat buffer and its Adam moments, [n_params]; m, v may be NULL for scoring */
    float *grad;                   /* [n_params] or NULL: receives the gradient of the LAST step when apply_update == 0 */
    float *logits_out;             /* [batch * n_items] or NULL: a copy of the LAST step's logits before dl overwrites them */
    float dropout, anneal_cap, lr, beta1, beta2, adam_eps;
    int64_t total_anneal_steps;
    uint64_t seed;
    int64_t ws_nnz_cap;            /* the (batch, nnz_cap) the workspace was laid out for */
    int32_t ws_batch, reserved;
    void *workspace;
    int64_t workspace_bytes;
} rk_mvae_desc;
/* *out = the layout for steps of up to `batch` users holding up to nnz_cap stored entries.  Host only, nothing launched.
 * RK_EINVAL: n_items outside 1..RK_MVAE_MAX_ITEMS, hidden outside 1..RK_MVAE_MAX_HIDDEN, latent outside 1..RK_MVAE_MAX_LATENT,
 * batch outside 1..RK_MVAE_MAX_BATCH, nnz_cap outside 1..2^31 - 1, no `out`. */
int rk_mvae_workspace(int32_t n_items, int32_t hidden, int32_t latent, int32_t batch, int64_t nnz_cap, rk_mvae_layout *out);
/* One epoch over user_ids[0 .. n): ceil(n / batch) steps as defined, the first with step = step0; every stage of the LAST step
 * stays readable in the workspace.  A check kernel that reads only the ids and the rating rows runs first and status (device,
 * int32[2]) is read back, the call's only synchronisation: {0, -1} without a violation; with one RK_EINVAL, status =
 * {RK_MVAE_*, lowest offending position (or step)} and nothing else is launched or written.  losses[3 s .. 3 s + 2] = {loss,
 * mean nll, mean KL} of step s (device, double).  With apply_update == 0 the parameters and moments are not touched and
 * desc->grad receives the gradient.  RK_EINVAL with nothing launched and nothing written: the limits of rk_mvae_workspace, a
 * workspace smaller than its layout or not aligned to 256 bytes, batch above ws_batch, n < 1, step0 < 0, dropout outside
 * [0, 1), anneal_cap negative or not finite, a missing pointer, apply_update == 0 without desc->grad. */
int rk_mvae_train_epoch(const rk_mvae_desc *desc, const int32_t *user_ids, int64_t n, int32_t batch, int64_t step0,
                        int32_t apply_update, double *losses /*[3*n_steps]*/, int32_t *status /*int32[2]*/, void *stream);
/* out[r * ldo + i] = the inference logit of item i for user_ids[r], r < nb, seen items included, written by the GEMM's
 * epilogue in blocks of ws_batch rows.  The ids are range-checked first (one synchronisation); a bad one is RK_EINVAL. */
int rk_mvae_scores(const rk_mvae_desc *desc, const int32_t *user_ids, int32_t nb, float *out, int64_t ldo, void *stream);
/* out[q] = the inference logit of (user_ids[q], item_ids[q]), q < n: the same chain order, so a pair equals the entry of
 * rk_mvae_scores to the bit.  n == 0 does nothing; ids outside the tables are RK_EINVAL. */
int rk_mvae_pair_scores(const rk_mvae_desc *desc, const int32_t *user_ids, const int32_t *item_ids, int64_t n, float *out,
                        void *stream);

/* ---------------------------------------------------------------- attacker --------- */
/* AUSH (recad/model/attacker/aush.py, registry recad/default.py:159-168) without the dense U x I train_mat
 * (explicit.py:102,134-143) and the dense B x I batches (explicit.py:178-199, aush.py:92-134): each attack row is the sparse
 * set "fillers U S" of the rating CSR (rows sorted by item).  recad_amd/attack/aush.py drives these entries.  All
 * pointers are device pointers and calls are asynchronous on `stream` unless stated otherwise.  Random draws come from
 * rk_mix64 keyed on (seed, stream_id, row, draw). */
#define RK_AUSH_HG 128            /* generator hidden width, Linear(I, 128) (aush.py:213-218) */
#define RK_AUSH_HD 150            /* discriminator width, Linear(I, 150) and two Linear(150, 150) (aush.py:226-235) */
#define RK_AUSH_MAX_FILLER 256    /* filler_num limit */
#define RK_AUSH_MAX_SELECT 16     /* |selected_ids| limit */
#define RK_AUSH_MAX_PAIRS 4096    /* batch * |selected_ids| limit (the ZR selection of one batch runs in one workgroup) */

typedef struct rk_aush_desc {
    int32_t n_users, n_items, filler_num, n_sel, batch, reserved;
    const int32_t *rowptr, *col;   /* rating CSR [n_users + 1] / [nnz], item ids ascending inside a row */
    const float *val;              /* ratings [nnz] */
    const int32_t *sel;            /* selected_ids [n_sel] */
    const float *g_w1t, *g_b1;     /* generator Linear(I, 128): weight transposed (item-major [n_items, 128]), bias [128] */
    const float *g_w2, *g_b2;      /* generator Linear(128, I): weight [n_items, 128] (torch layout), bias [n_items] */
    float *d_param, *d_m, *d_v;    /* the discriminator packed in one buffer, Adam moments alike: W1 transposed (item-major
                                      [n_items, 150]), b1 [150], W2 [150, 150], b2, W3 [150, 150], b3, w4 [150], b4 [1] */
    uint8_t *touched;              /* [n_items], zero-initialised: first-layer rows that ever had a gradient */
    int32_t *touched_list;         /* [n_items]: those rows, in first-touch order */
    int32_t *n_touched;            /* [1], zero-initialised */
    int32_t *gslot;                /* [n_items], every entry -1 initially (and again after each step) */
    void *work;                    /* rk_aush_workspace_bytes(batch, filler_num, n_sel) bytes */
    int64_t work_bytes;
    float lr, beta1, beta2, eps;   /* D's torch.optim.Adam (lr_d, aush.py:34-37) */
} rk_aush_desc;

/* Workspace of rk_aush_d_step / rk_aush_train_epoch (host only, no HIP call). */
int rk_aush_workspace_bytes(int32_t batch, int32_t filler_num, int32_t n_sel, int64_t *bytes);
/* The filler pool of each user -- rated items (value > 0) outside excl (sorted, = selected_ids U target_id_list),
 * aush.py:63-70 -- as a CSR (pool_ptr [n_users + 1], pool_col [nnz]), and the users whose pool holds at least filler_num
 * items, ascending, in eligible[0..*n_eligible): filler_filter_mat (utils.py:192-196) and aush.py:177-180.  Synchronous;
 * *n_eligible is a host pointer. */
int rk_aush_eligible(int32_t n_users, const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *excl, int32_t n_excl,
                     int32_t filler_num, int32_t *pool_ptr, int32_t *pool_col, int32_t *eligible, int32_t *n_eligible, void *stream);
/* out = a permutation of in[0..n) by a radix sort of 64-bit random keys: np.random.permutation (explicit.py:189, aush.py:181). */
int rk_aush_permute(int32_t n, const int32_t *in, uint64_t seed, uint64_t stream_id, int32_t *out, void *stream);
/* sample_fillers (aush.py:60-77) for rows users[0..n_rows): filler_num draws with replacement from the user's pool (row index
 * row0 + r in the RNG key), or the item ids draws[n_rows, filler_num] when draws != NULL (replay).  Duplicates collapse: the
 * distinct fillers ascending in fcol[r, 0..nf[r]) with their ratings in fval (padding: item 2^31 - 1, rating 0); sval[r, s] =
 * the rating at sel[s] (0 when unrated). */
int rk_aush_sample(int32_t n_rows, const int32_t *users, int32_t filler_num, const int32_t *rowptr, const int32_t *col, const float *val,
                   const int32_t *pool_ptr, const int32_t *pool_col, const int32_t *draws, uint64_t seed, uint64_t stream_id, int64_t row0,
                   const int32_t *sel, int32_t n_sel, int32_t *fcol, float *fval, int32_t *nf, float *sval, void *stream);
/* ZR_mask (aush.py:114-119) per batch of `batch` consecutive rows: of the n pairs (row, s) with sval == 0, exactly
 * n - floor(n * (1 - zr_ratio)) (double arithmetic, as Python) get zr = 1, a uniform random subset. */
int rk_aush_zr(int32_t n_rows, int32_t batch, int32_t n_sel, const float *sval, double zr_ratio, uint64_t seed, uint64_t stream_id,
               uint8_t *zr, void *stream);
/* gen[r, s] = 5 sigma(W2[sel_s] . sigma(W1 template_r + b1) + b2[sel_s]), the generator (aush.py:211-222) at S only; the
 * template is the fillers of row r with their ratings (aush.py:126).  w1t is item-major [n_items, 128]. */
int rk_aush_gen(int32_t n_rows, int32_t filler_num, const int32_t *fcol, const float *fval, const int32_t *nf, const float *w1t,
                const float *b1, const float *w2, const float *b2, const int32_t *sel, int32_t n_sel, float *gen, void *stream);
/* One batch of Aush.train_step (aush.py:128-167) on B <= desc->batch sampled rows: the discriminator step on
 * real / fake = profile * (fillers_mask + selects_mask) with fake[S] = gen + 5 (target_patch at selected_ids, aush.py:121),
 * torch.optim.Adam step adam_t on D (first-layer gradient reduced in (item, row) order: bit-reproducible), then
 * losses[0..4) = d_loss, g_loss_rec, g_loss_shilling, g_loss_gan (with the updated D).  The generator is not changed
 * (aush.py:138 detaches it).  The replay entry: the sample may come from rk_aush_sample with given draws and a given zr.
 * Gradient read-out (the per-kernel tests rely on it): with desc->lr = 0, beta1 = beta2 = 0, eps > 0, d_m = d_v = 0 and
 * adam_t = 1 the Adam element computes m = 0 + 1 * (g - 0) and v = 0 * 0 + 1 * g * g with a step size of 0, so the call leaves
 * d_m = the gradient of every parameter exactly as the kernels summed it (first-layer rows outside the batch stay 0),
 * d_v = g * g, d_param unchanged bit for bit, and g_loss_gan evaluated with the unchanged D. */
int rk_aush_d_step(const rk_aush_desc *desc, int32_t B, const int32_t *fcol, const float *fval, const int32_t *nf, const float *sval,
                   const float *gen, const uint8_t *zr, int32_t adam_t, float *losses, void *stream);
/* One epoch of Aush.train_step without a host round trip: permutation of eligible[0..n_eligible) (stream_id = epoch), filler
 * draws, ZR masks and generator values for every row, then rk_aush_d_step per batch of desc->batch rows (the last one short),
 * Adam steps adam_t0 + 1, ...; losses [n_batches, 4].  Row buffers: perm, nf [n_eligible], fcol / fval [n_eligible, filler_num],
 * sval / gen / zr [n_eligible, n_sel]. */
int rk_aush_train_epoch(const rk_aush_desc *desc, const int32_t *eligible, int32_t n_eligible, const int32_t *pool_ptr,
                        const int32_t *pool_col, uint64_t seed, uint64_t epoch, double zr_ratio, int32_t adam_t0, int32_t *perm,
                        int32_t *fcol, float *fval, int32_t *nf, float *sval, float *gen, uint8_t *zr, float *losses, void *stream);
/* generate_fake's profiles (aush.py:187-206) into out [n_rows, n_items] (zero-filled first): the fillers' ratings, 5 at every
 * target of every row, and at S round-half-even(gen (+ 5 where s is a target)) clipped to [1, 5]; pre (optional,
 * [n_rows, n_sel]) receives the values before rounding. */
int rk_aush_fake_assemble(int32_t n_rows, int32_t n_items, int32_t filler_num, const int32_t *fcol, const float *fval, const int32_t *nf,
                          const int32_t *sel, int32_t n_sel, const float *gen, const int32_t *tgt, int32_t n_tgt, float *pre, float *out,
                          void *stream);

/* The heuristic attackers: average, segment and bandwagon (recad/model/attacker/heuristic.py:85-325, registry
 * recad/default.py:136-158).  recad_amd/attack/heuristic.py drives these entries.  Pointers are device memory unless a
 * comment says host. */
#define RK_HEUR_MAX_FILLER 256    /* filler_num limit (one workgroup draws a row's fillers) */
#define RK_HEUR_MAX_TARGETS 64    /* target ids per call */
#define RK_HEUR_MAX_SELECT 64     /* |selected_ids| limit */
#define RK_HEUR_GLOBAL 0          /* filler values: N(global mean, global std)  (bandwagon, heuristic.py:301-305) */
#define RK_HEUR_ITEM 1            /* N(item mean, item mean) for a rated item, N(global mean, global std) otherwise (average, :139-145) */
#define RK_HEUR_ONES 2            /* the value 1 (segment, heuristic.py:217) */
/* Rating statistics of the nnz stored ratings (col, val) of a rating CSR -- its row structure is not needed --, replacing
 * heuristic.py:91-98 (one mask over all ratings per distinct item) and the counting half of :245-258: item_count [n_items],
 * item_mean [n_items] float64 (0 where item_count is 0), global [2] = {mean, population std} of all ratings (np.mean / np.std;
 * {0, 0} when nnz is 0), n_rated [1] = the number of items with a rating.  All sums are float64.  The per-item sums are float64
 * atomics, so item_mean may differ between two runs at rounding level; the counts and global are the same on every run.
 * Asynchronous on the stream. */
int rk_heur_item_stats(int32_t n_items, int64_t nnz, const int32_t *col, const float *val, int32_t *item_count, double *item_mean,
                       double *global, int32_t *n_rated, void *stream);
/* The k most rated items, most rated first, replacing the groupby / sort_values / [::-1] / [:11] of heuristic.py:252-259 (whose
 * order among equal counts is the unstable sort's; here the larger item id comes first).  Selected on the integer counts.  An
 * item nobody rated is never returned: ids / counts [k] hold *n_found (host) <= k entries, then -1 / 0.  Synchronous. */
int rk_heur_popular(int32_t n_items, const int32_t *item_count, int32_t k, int32_t *ids, int32_t *counts, int32_t *n_found, void *stream);
/* generate_fake (heuristic.py:115-151, 191-220, 274-311): out [attack_num, n_items], every element written.  targets
 * [n_targets] and selected [n_sel] are HOST arrays.  With rate = attack_num / n_targets (integer), row r < rate * n_targets
 * rates targets[r / rate] with 5 and the other rows rate no target (none does when rate is 0): the reference's slices.  Every
 * row rates every selected id 5 and filler_num distinct items outside targets U selected, uniformly drawn, with the mode's
 * value: a normal one is rounded half to even, then clipped to [1, 5].  item_mean / item_count (rk_heur_item_stats) are read
 * in the ITEM mode only.  The replay form: draw_cols [attack_num, filler_num] (item ids, distinct and outside targets U
 * selected in each row: the caller's duty) and draw_vals (the float64 values before rounding; not needed in the ONES mode)
 * replace every draw.  RK_EINVAL, with nothing launched or written: an id outside [0, n_items), a size outside the limits
 * above, fewer than filler_num items outside targets U selected, an unknown mode. */
int rk_heur_generate(int32_t attack_num, int32_t n_items, int32_t filler_num, const int32_t *targets, int32_t n_targets,
                     const int32_t *selected, int32_t n_sel, int32_t mode, double global_mean, double global_std,
                     const double *item_mean, const int32_t *item_count, const int32_t *draw_cols, const double *draw_vals,
                     uint64_t seed, uint64_t stream_id, float *out, void *stream);

/* UBA's target-user budget selection (recad/model/attacker/uba.py:81-140, registry recad/default.py:210-221); its GAN is AUSH's
 * and uses the rk_aush_* entries.  recad_amd/attack/uba.py drives these entries.  target_users [n_targets] is a HOST array;
 * every other pointer is device memory unless a comment says host.  A budget step b = 1..budget is the reference's add_num: the
 * number of copies of each redrawn row it appends (uba.py:92-93, 123).  The redrawn rows of one (b, trial) are a side CSR over
 * the target users in the caller's order: side_ptr [n_targets + 1], side_col / side_val [side_cap] (item ids ascending; int32
 * ratings), where side_cap >= the target users' ratings + one entry per target user who has not rated s.
 * RK_EINVAL with nothing launched or written: no or more than RK_UBA_MAX_TARGETS target users, one listed twice or outside
 * [0, n_users), s outside [0, n_items), b or budget outside 1..RK_UBA_MAX_BUDGET, side_cap outside [n_targets, n_targets *
 * n_items], an unknown mode or path, RK_UBA_PATH_LDS with n_users above RK_UBA_LDS_USERS, and in the MATRIX mode a shape whose
 * scores can exceed 2^53 ((n_users + n_targets * b) * 125 * n_items: sums are int64 and leave as exact doubles). */
#define RK_UBA_MAX_BUDGET 16      /* budget limit (uba.py:182 reads 6 columns whatever the budget; the build reads `budget`) */
#define RK_UBA_MAX_TARGETS 64     /* target users per call: one lane of a wave each in the gather */
#define RK_UBA_TRIALS 10          /* redraws per budget step (uba.py:127) */
#define RK_UBA_TOPN 10            /* the top-N the selected item must reach (uba.py:102) */
#define RK_UBA_LDS_USERS 8000     /* n_users up to which a target user's weight vector is kept in LDS (8 bytes each) */
#define RK_UBA_ELEMENTWISE 0      /* scores = the redrawn row cubed elementwise: uba.py:99 as written */
#define RK_UBA_MATRIX 1           /* scores = rows target_user_ids of (E @ E @ E)[:M, M:], E the expanded (M+N)^2 matrix (uba.py:95-98) */
#define RK_UBA_PATH_AUTO 0        /* LDS when n_users <= RK_UBA_LDS_USERS, else WORK */
#define RK_UBA_PATH_LDS 1         /* weight vectors accumulated and staged in LDS */
#define RK_UBA_PATH_WORK 2        /* weight vectors accumulated with global atomics in the scratch, read from there */
/* The stream-ordered scratch one rk_uba_prob call takes (rk_uba_scores takes the same with budget 1): side CSR, counters, the
 * weight vectors [n_targets, n_users] int64 and the score rows [n_targets, n_items] float64.  Host only, no HIP call. */
int rk_uba_workspace_bytes(int32_t n_users, int32_t n_items, int32_t n_targets, int32_t side_cap, int32_t budget, int64_t *bytes);
/* uba.py:86-91 for one (b, trial): every target user's rated items (rowptr / col of the rating CSR with nnz entries, item ids
 * ascending inside a row) each get an integer uniform in 1..5 -- from rk_mix64 keyed on (seed, b, trial, target index, position
 * in the side row), or draws[side position] when draws != NULL (replay; laid out like side_val, the entry at s is ignored) --
 * and s gets 5, inserted in order when the user had not rated it.  The rating CSR is only read.  *status (device, zeroed by
 * the caller) becomes 1, and nothing else is written, when the rows need more than side_cap entries or a row pointer is out of
 * order.  Asynchronous. */
int rk_uba_redraw(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *target_users,
                  int32_t n_targets, int32_t s, int32_t b, int32_t trial, const int32_t *draws, uint64_t seed, int32_t side_cap,
                  int32_t *side_ptr, int32_t *side_col, int32_t *side_val, int32_t *status, void *stream);
/* uba.py:95-113 for one redraw as counts: with x_t target user t's score row, counts [3, n_targets] = n_greater = #{j : x_t[j] >
 * x_t[s]}, n_equal = #{j != s : x_t[j] == x_t[s]}, n_equal_before = the equal ones with j < s; x (optional, [n_targets, n_items]
 * float64) receives the score rows.  ELEMENTWISE: x_t = the redrawn row cubed.  MATRIX: x_t = sum_v c_v <r'_v, r'_t> r'_v over
 * all users v of the rating CSC (colptr [n_items + 1], crow / cval [nnz], the transpose of the rating CSR; ratings are
 * integers), a target user's row taken from the side CSR instead, c_v = 1 + b for a target user and 1 otherwise: the
 * reference's expanded matrix with its b appended copies per target user, none of it materialised.  Integer arithmetic: exact,
 * the same on every run.  Asynchronous. */
int rk_uba_scores(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *colptr, const int32_t *crow, const float *cval,
                  const int32_t *target_users, int32_t n_targets, const int32_t *side_ptr, const int32_t *side_col, const int32_t *side_val,
                  int32_t side_cap, int32_t s, int32_t b, int32_t mode, int32_t path, int32_t *counts, double *x, void *stream);
/* budget_matrix (uba.py:119-140): for b = 1..budget and RK_UBA_TRIALS trials each, redraw, score and count a hit when
 * n_greater + n_equal_before < RK_UBA_TOPN; prob_mat [n_targets, budget] (HOST, float64) = hits / RK_UBA_TRIALS and *n_tie
 * (HOST) = the number of (b, trial, target user) cases with n_greater < RK_UBA_TOPN <= n_greater + n_equal, where the
 * reference's np.argsort leaves the answer to the order among equal scores.  draws: NULL, or [budget, RK_UBA_TRIALS, side_cap]
 * replayed draws, each slab laid out like side_val.  Synchronous: one read-back at the end.  RK_EINVAL also when the rows do
 * not fit side_cap. */
int rk_uba_prob(int32_t n_users, int32_t n_items, int64_t nnz, const int32_t *rowptr, const int32_t *col, const int32_t *colptr,
                const int32_t *crow, const float *cval, const int32_t *target_users, int32_t n_targets, int32_t s, int32_t budget,
                int32_t mode, int32_t path, const int32_t *draws, uint64_t seed, int32_t side_cap, double *prob_mat, int32_t *n_tie,
                void *stream);

/* AIA (recad/model/attacker/aia.py, registry recad/default.py:169-186): the weighted-MF surrogate trained from scratch on every
 * train_step, the reverse pass through its unrolled Adam steps, the attack loss and the generator's Adam step.  The surrogate's
 * data is one CSR of R = n_real + fake rows (the rating CSR, then filler_num slots per fake row holding the projected generator),
 * item ids ascending inside a row; weight_neg_s is 0, so an entry weighs w_pos when X > 0 and nothing otherwise.  Its state
 * is [P (R rows); Q (n_items rows)], each row dpad floats (d padded with zero columns); a SLOT is theta, m, v of that shape,
 * 3 (R + n_items) dpad floats.  Step j of an epoch trains the rows perm[j * batch .. min((j + 1) * batch, R)).  recad_amd/attack/
 * aia.py drives these entries; all pointers are device pointers and calls are asynchronous on `stream`.  No float atomics:
 * every result is bit-reproducible. */
#define RK_AIA_MAX_BATCH 256      /* batch_size_s limit */

typedef struct rk_aia_desc {
    int32_t n_rows, n_real, n_items, dpad, batch, n_fake_nz;
    int64_t nnz_real;              /* the fake rows' entries start here in col / x */
    const int32_t *rowptr, *col;   /* [n_rows + 1] / [nnz_real + n_fake_nz] */
    const float *x;                /* [nnz_real + n_fake_nz]: ratings, then the projected generator (rk_aia_project) */
    float lr, beta1, beta2, eps, wd, w_pos;   /* the surrogate's torch.optim.Adam(lr_s, weight_decay=weight_decay_s), weight_pos_s */
} rk_aia_desc;

/* x[k] = clamp(round_half_even(gen[k]), 0, 5) (project, aia.py:534-549). */
int rk_aia_project(int32_t n, const float *gen, float *x, void *stream);
/* Steps lo .. hi-1 of one epoch of the surrogate (aia.py:444-461), Adam steps adam_t_lo, adam_t_lo + 1, ...: batch loss
 * sum_r sum_i w (X_ri - p_r . q_i)^2 over the batch's positives, weight decay on every row, one launch per step.  keep_all:
 * step lo + k reads slot k of `slots` and writes slot k + 1 (hi - lo + 1 slots); otherwise two slots, step lo + k reads slot
 * (parity0 + k) & 1 and writes the other.  adam_t_lo is the 1-based Adam step number of step lo itself (the first step of a fresh
 * surrogate has adam_t 1; adam_t_lo < 1 is refused), counted across epochs.  A stored entry with X <= 0 weighs nothing but is
 * still searched; slot k is only read, and no slot other than the ones named is touched.  RK_EINVAL (nothing launched): dpad not
 * 16 / 32 / 64, batch outside [1, RK_AIA_MAX_BATCH], n_real > n_rows, lo > hi, hi beyond ceil(n_rows / batch), parity0 not 0 / 1,
 * a null pointer. */
int rk_aia_forward(const rk_aia_desc *desc, const int32_t *perm, const int32_t *invperm, int32_t lo, int32_t hi, int32_t adam_t_lo,
                   float *slots, int32_t keep_all, int32_t parity0, void *stream);
/* The reverse of steps hi-1 down to lo (the unrolled epoch, aia.py:463-482): slots as rk_aia_forward's keep_all (slot k = the
 * input of step lo + k).  adj [3 slots' worth: theta-bar, m-bar, v-bar] is updated in place from the adjoint of step hi's
 * output to that of step lo's input; gbar [(R + n_items) dpad] is scratch; xbar [n_fake_nz] accumulates dF/dX of the fake
 * entries (zero it before the first call).  Where v' == 0 exactly, the 1 / sqrt(v') term of v-bar is taken as 0.  adam_t_lo is
 * the Adam step number of step lo, as in rk_aia_forward (step lo + k is reversed with adam_t_lo + k).  Of slot k + 1 only m' and v'
 * are read.  After a one-step call gbar holds the adjoint of that step's gradient (g-bar = (1 - b1) m-hat + 2 (1 - b2) g v-hat).
 * xbar may be null when n_fake_nz is 0 or there is no fake row.  A range equals its single steps run from hi - 1 down, bit for bit. */
int rk_aia_reverse(const rk_aia_desc *desc, const int32_t *perm, const int32_t *invperm, int32_t lo, int32_t hi, int32_t adam_t_lo,
                   const float *slots, float *adj, float *gbar, float *xbar, void *stream);
/* G_loss (aia.py:88-114) of theta = P Q^T into loss[0] and its gradient into adj (zeroed first; P rows of real users and Q rows
 * set, m-bar / v-bar zero).  Pairs (user, target) with train_mat[u, t] == 0, grouped by target: pair_ptr [n_tgt + 1],
 * pair_user / pair_tgt (item id) / pair_slot (target index) [n_pairs]; pidx [n_tgt, n_real] = the pair index or -1; tscale
 * [n_tgt] = 1 / (11 |T_t|) (as float).  work: 3 n_pairs floats (scratch).  The rows of adj that belong to fake users (n_real ..
 * n_rows - 1) stay 0: only real users are pairs.  An item i != t with s_ui == s_ut exactly is inside the mask (>=).  Scores are
 * shifted by their running maximum before expf, so scores beyond expf's range give a finite loss.  n_tgt <= 0 or n_pairs <= 0 is
 * refused. */
int rk_aia_attack_loss(const rk_aia_desc *desc, int32_t n_tgt, const int32_t *tgt, const int32_t *pair_ptr, int32_t n_pairs,
                       const int32_t *pair_user, const int32_t *pair_tgt, const int32_t *pair_slot, const int32_t *pidx,
                       const float *tscale, const float *theta, float *work, float *loss, float *adj, void *stream);
/* torch.optim.Adam step adam_t (no weight decay) on gen [n] with gradient grad: the G optimizer (aia.py:22-37, 66-68). */
int rk_aia_g_step(int32_t n, float *gen, float *m, float *v, const float *grad, int32_t adam_t, float lr, float beta1, float beta2,
                  float eps, void *stream);

/* AushPlus (recad/model/attacker/aushplus.py, registry recad/default.py:187-209): the discretising autoencoder generator
 * DiscretGenerator_AE_1(p_dims = [n_items, 125]) and the Discriminator (n_items -> 512 -> 128 -> 1), on CSR rows only: every
 * consumer of the generator reads it where the input row is non-zero, so nothing rows x n_items is formed.  recad_amd/attack/
 * aushplus.py drives these entries (and rk_aia_* for the surrogate, rk_adam_step for the optimisers).  No float atomics.
 * Packed generator parameters (and gradients), float32:
 *   w1t [n_items, RK_AP_HG] (layers.0.weight transposed, hidden 125 padded with zeros) | b1 [RK_AP_HG] | w2 [n_items, RK_AP_HG]
 *   (layers.1.weight, padded) | b2 [n_items] | min_boundary_value [n_items] | interval_lengths [n_items, 3]
 * Packed discriminator parameters (and gradients):
 *   w1t [n_items, RK_AP_HD1] (main.0.weight transposed) | b1 [RK_AP_HD1] | W2 [RK_AP_HD2, RK_AP_HD1] | b2 [RK_AP_HD2] | w3 [RK_AP_HD2] | b3 [1] */
#define RK_AP_HG 128
#define RK_AP_HG_REAL 125
#define RK_AP_HD1 512
#define RK_AP_HD2 128
#define RK_AP_G_FLOATS(I) ((int64_t)(I) * (2 * RK_AP_HG + 5) + RK_AP_HG)
#define RK_AP_D_FLOATS(I) ((int64_t)(I) * RK_AP_HD1 + RK_AP_HD1 + (int64_t)RK_AP_HD2 * RK_AP_HD1 + 2 * RK_AP_HD2 + 1)
/* floats of rk_ap_d_step's work per row: h1, dz1 [RK_AP_HD1 each], h2, dz2 [RK_AP_HD2 each], p, dlogit, weighted row loss; stored
 * array by array over the n rows in that order */
#define RK_AP_D_WORK_PER_ROW (2 * RK_AP_HD1 + 2 * RK_AP_HD2 + 3)

/* Generator forward (aushplus.py:425-447, 311-378) over rows rowptr[0 .. n_rows] of a CSR (rowptr holds offsets into col / x and
 * into the per-entry outputs): norm [n_rows] = max(||x_r||, 1e-12), h1 [n_rows, RK_AP_HG] = relu(W1 x_r / norm + b1), and per
 * stored entry k = (r, j): a = 2.5 tanh(W2_j . h1 + b2_j) + 2.5, cls = the class c in 0..4 whose four Heaviside factors all
 * hold (-1 when a sits exactly on a boundary: the all-zero distribution), value = (cls + 1) [x > 0]. */
int rk_ap_g_forward(int32_t n_rows, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *x, const float *gparam,
                    float *norm, float *h1, float *a, int32_t *cls, float *value, void *stream);
/* Generator backward into ggrad (packed; every element written).  mode 0: from dvalue = dL/dvalue per entry (taken where
 * x > 0); mode 1: from CrossEntropyLoss of the five 0/1 products against x - 1 over the entries with x > 0, scale = 1 / their
 * number, loss[0] = that mean.  The Heaviside's backward is dy (1 - tanh^2) (HeaviTanh, aushplus.py:192-224).  tptr [n_items + 1],
 * tent, trow: the rows' entries grouped by item in a fixed order (entry index into col / x, row index relative to rowptr).
 * Scratch: zbar, eloss [per entry, indexed like col], bbar [4 per entry], dpre [n_rows, RK_AP_HG]; entry0 = rowptr[0] and
 * n_entries = rowptr[n_rows] - rowptr[0] as the host knows them (mode 1 sums eloss over that range in a fixed order). */
int rk_ap_g_backward(int32_t n_rows, int32_t n_items, const int32_t *rowptr, const int32_t *col, const float *x, const float *gparam,
                     const float *norm, const float *h1, const float *a, int32_t mode, const float *dvalue, float scale,
                     int64_t entry0, int64_t n_entries, const int32_t *tptr, const int32_t *tent, const int32_t *trow, float *zbar, float *bbar,
                     float *eloss, float *dpre, float *ggrad, float *loss, void *stream);
/* Discriminator forward, nn.BCELoss and backward (aushplus.py:103-131, 57-60) on nA rows of CSR A (label labelA) followed by nB
 * rows of CSR B (labelB): loss[0] = mean_A BCE + mean_B BCE.  dgrad (optional, packed, every element written) needs the
 * entries of all n = nA + nB rows grouped by item: tptr [n_items + 1], trow (row in 0..n), tsrc (index into valA for an A row,
 * into valB for a B row).  dinB (optional) receives dL/dvalB at B's entries.  work: n * RK_AP_D_WORK_PER_ROW floats. */
int rk_ap_d_step(int32_t n_items, int32_t nA, const int32_t *rowptrA, const int32_t *colA, const float *valA, float labelA, int32_t nB,
                 const int32_t *rowptrB, const int32_t *colB, const float *valB, float labelB, const float *dparam, float *work,
                 const int32_t *tptr, const int32_t *trow, const int32_t *tsrc, float *dgrad, float *dinB, float *loss, void *stream);
/* What the kernel tests hold the three entries to (tests/_aushplus_stages.py counts every rounding; u = 2^-24, T = 4 the allowance
 * of tanhf / expf / logf from the HIP math API's accuracy table, doubled), each stage against float64 on the stage's own inputs as
 * they stand in the caller's buffers.  G forward: norm (K / 2 + 2) u norm over a row of K entries, exactly 1e-12f for an empty or
 * all-zero row; h1 (K + 4) u (sum|x w| / norm + |b1|); a: the logit's (128 + 8) u (sum|w h| + |b2|) through 2.5 tanh, plus
 * (T + 2) u 2.5 |tanh z| + u |a|; cls and value from a: bits (boundaries, differences and the four strict comparisons in fp32,
 * nothing contracted).  G backward: bbar, zbar, eloss from a within the sum of the roundings of tanhf(a - b_k), 1 - th^2, the sums
 * over the classes, mode 1's expf / logf and h2 = (a - 2.5) / 2.5; dpre (K + 2) u sum|zbar w2|, +0.0 where h1 <= 0; the w2 and w1t
 * rows of an item with n_j entries (n_j + 2) u and (n_j + 3) u sum|terms|.  D: h1 (K + 2) u, h2 (512 + 8) u, the logit (128 + 8) u
 * (sum|terms| + |bias|); p additionally (T + 2) u p; from p, rowloss within (T + 2) u relative plus u / n_side (the rounding of
 * 1 - p) and dlogit within 10 u relative; dz2 one product:
 * bits; dz1 (128 + 2) u, dinB (512 + 8) u, W2-bar and w3-bar (n + 2) u, an item's w1t row (n_j + 2) u sum|terms|.
 * Bit-exact orders (additions only, nothing to contract): the b2, min_boundary and interval_lengths gradients (a chain over the
 * item's list; per entry ((bbar0 + bbar1) + bbar2) + bbar3 and its tails), G's b1-bar (dpre over the rows in row order), D's b1, b2
 * and b3 gradients (rows in row order), and loss[0] of both entries (256 strided partials, then the halving tree).
 * A stored entry with x <= 0 gets a, cls and zero value like any other, contributes to norm and h1, and takes no part in mode 1:
 * its eloss, zbar and bbar are zero and scale does not count it; in mode 0 its dvalue is ignored.  Empty rows are allowed
 * everywhere (G: h1 = relu(b1), norm = 1e-12f; D: h1 = relu(b1)).  A call on rows rowptr[0 .. n_rows] writes a, cls, value, zbar,
 * bbar, eloss only at entries rowptr[0] .. rowptr[n_rows] - 1 and norm, h1, dpre only at rows 0 .. n_rows - 1, dinB only at B's
 * entries; everything outside is untouched.  ggrad and dgrad are written in full: items no listed entry touches, the hidden padding
 * lanes 125 .. 127, interval lengths <= 0 and units behind a closed relu get +0.0.  With p saturated to exactly 0 or 1 the row loss
 * is 0 or 100 / n_side (nn.BCELoss's clamp) and dlogit is 0.  A refused call (RK_EINVAL) has launched and written nothing;
 * rk_ap_g_forward with n_rows == 0 is an empty call (RK_OK); nA == 0 or nB == 0 (not both) and dgrad == NULL or dinB == NULL are
 * forms of rk_ap_d_step, the absent side's pointers and the lists may then be NULL. */

#ifdef __cplusplus
}
#endif
#endif /* RECAD_HIP_H */
