"""The LDS-resident sliced SpMM (recad_amd/csrc/spmm_lds.h) restated in numpy from its PLAN alone: the walk of the plan in the
kernel's own summation order (tasks -> chunk partials -> per-row sums -> dinv scaling), the epilogues of rk_spmm_lds, the sliced
layout, and the seeded graphs at which every loop of the kernel takes every branch.  Shared by the host tests
(test_lds_plan_cpu.py, test_spmm_lds_forms_host.py), the GPU tests (test_spmm_lds_forms_gpu.py) and tools/spmm_lds_stress.py.

Every fp32 operation below is one numpy float32 operation, i.e. one rounding, in the order the kernel performs it:
  table[perm[c]] = fl(x[c] * dinv[c]);  partial = ((0 + t0) + t1) + ... in stream order;  acc = ((0 + p0) + p1) + ... in chunk order;
  y0 = fl(acc * dinv[r]).
No operation of that chain can contract into an FMA (a product stored to LDS, additions only, one product), so the kernel's y
must equal y0 bit for bit."""
import ctypes as C
import types

import numpy as np

from recad_amd import _lib

U32 = 2.0 ** -24      # unit roundoff of fp32

H = dict(MAGIC=0, NWG=1, U=2, I=3, D=4, LSU=5, LSI=6, NBLK0=7, NBLK1=8, WG_OFS=9, BLK_OFS=10, DINV_OFS=11, LDS_BYTES=12,
         CHUNK=13, NWORDS=14, PERM0=15, PERM1=16, MQ_OFS=17, WGX_OFS=18)
LB = dict(ROW0=0, NROWS=1, NPART=2, NTASKS=3, TASK_OFS=4, DST_OFS=5, PP_OFS=6, STREAM_OFS=7, WORDS=8)

# (slice_items, slice_users) of every (lpa, lpb) pair spmm_lds_launch / spmm_lds_multi_launch dispatch to: lp = width / 4
FORMS = {(1, 1): (4, 4), (1, 2): (4, 8), (2, 1): (8, 4), (2, 2): (8, 8), (4, 4): (16, 16), (4, 2): (16, 8), (2, 4): (8, 16)}


def norm_adj_csr(U, I, ptr, idx):
    """rowptr, col, val (float32, val = dinv[r]*dinv[c] like implicit.py:259-277) of the bipartite adjacency."""
    N = U + I
    users = np.repeat(np.arange(U), np.diff(ptr))
    items = idx.astype(np.int64)
    rows = np.concatenate([users, U + items])
    cols = np.concatenate([U + items, users])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    deg = np.bincount(rows, minlength=N)
    rowptr = np.zeros(N + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(deg)
    with np.errstate(divide="ignore"):
        dinv = np.where(deg > 0, 1.0 / np.sqrt(deg.astype(np.float64)), 0.0).astype(np.float32)
    val = (dinv[rows] * dinv[cols]).astype(np.float32)
    return rowptr, cols.astype(np.int32), val


def build_plan_handle(U, I, rowptr, col, val, dim, n_cu=256, form=None, cap=0):
    """(plan handle or None, info, rc): form = (slice_items, slice_users) floats, cap = chunk cap; None / 0 = the shipped
    choice through rk_lds_plan_build_host itself, anything else through rk_lds_plan_build_host_ex.  The caller destroys."""
    plan, n_words, info = C.c_void_p(), C.c_int64(0), _lib.LdsInfo()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    cc = np.ascontiguousarray(col, dtype=np.int32)
    vv = None if val is None else np.ascontiguousarray(val, dtype=np.float32)
    args = (U, I, rp.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), None if vv is None else vv.ctypes.data_as(C.c_void_p), dim, n_cu)
    tail = (C.byref(plan), C.byref(n_words), C.byref(info))
    if form is None and not cap:
        rc = _lib.lib().rk_lds_plan_build_host(*args, *tail)
    else:
        si, su = form if form is not None else (0, 0)
        rc = _lib.lib().rk_lds_plan_build_host_ex(*args, si, su, cap, *tail)
    if rc != 0 or n_words.value == 0:
        return None, info, rc, 0
    return plan, info, rc, int(n_words.value)


def plan_words(plan, n_words):
    words = np.zeros(n_words, dtype=np.int32)
    _lib.check(_lib.lib().rk_lds_plan_words(plan, words.ctypes.data_as(C.c_void_p)), "rk_lds_plan_words")
    return words


def build_plan(U, I, rowptr, col, val, dim, n_cu=256, form=None, cap=0):
    plan, info, rc, n_words = build_plan_handle(U, I, rowptr, col, val, dim, n_cu, form, cap)
    assert rc == 0, _lib.lib().rk_last_error()
    if plan is None:
        return None, info
    words = plan_words(plan, n_words)
    _lib.lib().rk_lds_plan_destroy(plan)
    return words, info


B128_GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
               [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59], [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63])


def block_desc(words, half, rb):
    return words[int(words[H["BLK_OFS"]]) + ((int(words[H["NBLK0"]]) if half else 0) + rb) * LB["WORDS"]:][: LB["WORDS"]]


def walk(words, x, check_banks=True, strict=True):
    """The plan walked the way spmm_lds_kernel consumes it; x row-major [N, d] float32.  Returns a namespace:
    acc [N, d] fp32 -- the row sums before dinv[r];  y0 = fl(acc * dinv[r]);  entries -- live stream entries (per slice);
    dinv [N] fp32.  Every (half, slice, block) workgroup of the launch table is accounted for; the stream of a block is the
    same for all its slices, so a block is walked once over all d columns (the order per element is the slice's own).
    strict = False: for MUTATED plans -- the coverage assertions that a mutation breaks on purpose are skipped."""
    U, I, d = int(words[H["U"]]), int(words[H["I"]]), int(words[H["D"]])
    N = U + I
    S = {0: 1 << int(words[H["LSI"]]), 1: 1 << int(words[H["LSU"]])}   # half 0 gathers the items table
    dinv = words[int(words[H["DINV_OFS"]]): int(words[H["DINV_OFS"]]) + N].view(np.float32)
    stream16 = words.view(np.uint16)
    acc_out = np.full((N, d), np.nan, dtype=np.float32)
    seen_rows = np.zeros((N, d), dtype=np.int32)
    wg = words[int(words[H["WG_OFS"]]): int(words[H["WG_OFS"]]) + 4 * int(words[H["NWG"]])].reshape(-1, 4)
    nblk = {0: int(words[H["NBLK0"]]), 1: int(words[H["NBLK1"]])}
    # the launch table holds every (half, slice, block) exactly once
    want = sorted((h, s, rb) for h in (0, 1) for s in range(d // S[h]) for rb in range(nblk[h]))
    assert sorted((int(h), int(s), int(rb)) for h, s, rb, _ in wg) == want
    entries = 0
    for half in (0, 1):
        Sh = S[half]
        LPn = Sh // 4
        SL = 64 // LPn
        K = 16 // LPn
        n_src = U if half else I
        src0 = 0 if half else U
        dst0 = U if half else 0
        table = np.zeros((n_src + K, d), dtype=np.float32)
        perm = words[int(words[H["PERM1" if half else "PERM0"]]):][:n_src]
        assert np.array_equal(np.sort(perm), np.arange(n_src))
        table[perm] = x[src0: src0 + n_src] * dinv[src0: src0 + n_src, None]
        for rb in range(nblk[half]):
            bd = block_desc(words, half, rb)
            part = np.zeros((max(int(bd[LB["NPART"]]), 1), d), dtype=np.float32)
            written = np.zeros(part.shape[0], dtype=np.int32)
            for t in range(int(bd[LB["NTASKS"]])):
                ofs, nb = (int(v) for v in words[int(bd[LB["TASK_OFS"]]) + 2 * t: int(bd[LB["TASK_OFS"]]) + 2 * t + 2])
                dst = words[int(bd[LB["DST_OFS"]]) + t * SL: int(bd[LB["DST_OFS"]]) + (t + 1) * SL]
                base = (int(bd[LB["STREAM_OFS"]]) + ofs) * 8
                blk = stream16[base: base + nb * SL * 8].reshape(nb, SL, 8).astype(np.int64)
                assert blk.max(initial=0) < n_src + K
                if check_banks:
                    # every ds_read_b128 of the walk is conflict-free: the K slots of a 16-lane group read K different
                    # bank classes (row index mod K)
                    for grp in B128_GROUPS:
                        slots = sorted({lane // LPn for lane in grp})
                        cl = blk[:, slots, :] % K                       # [nb, K, 8]
                        srt = np.sort(cl, axis=1)
                        assert (srt[:, 1:, :] != srt[:, :-1, :]).all()
                acc = np.zeros((SL, d), dtype=np.float32)
                for b in range(nb):
                    for e in range(8):
                        acc = acc + table[blk[b, :, e]]
                entries += int((blk < n_src).sum())
                live = dst >= 0
                if strict:
                    assert (blk[:, ~live, :] >= n_src).all()      # empty slots only read zero rows
                part[dst[live]] = acc[live]
                written[dst[live]] += 1
            if strict:
                assert (written[: int(bd[LB["NPART"]])] == 1).all()
            n_rows = int(bd[LB["NROWS"]])
            pp = words[int(bd[LB["PP_OFS"]]): int(bd[LB["PP_OFS"]]) + n_rows + 1]
            racc = np.zeros((n_rows, d), dtype=np.float32)
            cnt = np.diff(pp)
            for k in range(int(cnt.max(initial=0))):              # k-th partial of every row that has one: chunk order per row
                rows = np.nonzero(cnt > k)[0]
                racc[rows] = racc[rows] + part[pp[rows] + k]
            r0 = dst0 + int(bd[LB["ROW0"]])
            acc_out[r0: r0 + n_rows] = racc
            seen_rows[r0: r0 + n_rows] += 1
    assert (seen_rows == 1).all()     # every (row, column) of the output is produced by exactly one workgroup
    return types.SimpleNamespace(acc=acc_out, y0=acc_out * dinv[:, None], entries=entries, dinv=dinv.copy())


def emulate(words, x, check_banks=True):
    """y = A.x computed the way spmm_lds_kernel does, from the plan alone.  x, y: row-major [N, d] float32."""
    w = walk(words, x, check_banks)
    return w.y0, w.entries


def product64(rowptr, col, val, x):
    """(float64 product with the STORED values, sum |val x| per element, nnz per row)"""
    N = len(rowptr) - 1
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    t = val.astype(np.float64)[:, None] * x[col].astype(np.float64)
    ref = np.zeros((N, x.shape[1]), dtype=np.float64)
    sabs = np.zeros_like(ref)
    np.add.at(ref, rows, t)
    np.add.at(sabs, rows, np.abs(t))
    return ref, sabs, np.diff(rowptr).astype(np.int64)


def budget_ratio(y, ref, sabs, nnz):
    """per element |y - ref| / ((nnz_r + 5) u sum|val x|): nnz products (against the stored value's one rounding: the two dinv
    factors, each rounded, and their two products -- the + 5 with the row's final scaling) and nnz - 1 additions, first order.
    0 where both sides are exactly zero (empty rows)."""
    err = np.abs(y.astype(np.float64) - ref)
    bud = (nnz[:, None] + 5) * U32 * sabs
    return np.where(err == 0, 0.0, err / np.where(bud > 0, bud, 1e-300))


# ---------------------------------------------------------------------------------------------- layout
def sl_off(info, r, k):
    """float offset of element (node r, column k) of a sliced [U+I, d] buffer (spmm_lds.h: sl_off), vectorised"""
    U, I, d, lsu, lsi = info.n_users, info.n_items, info.dim, info.lsu, info.lsi
    r, k = np.asarray(r, dtype=np.int64), np.asarray(k, dtype=np.int64)
    users = (((k >> lsu) * U + r) << lsu) + (k & ((1 << lsu) - 1))
    items = U * d + (((k >> lsi) * I + (r - U)) << lsi) + (k & ((1 << lsi) - 1))
    return np.where(r < U, users, items)


def sl_index(info):
    """flat sliced offset of every (r, k) as an [N, d] array: sliced.ravel()[sl_index] is the row-major view"""
    N, d = info.n_users + info.n_items, info.dim
    idx = sl_off(info, np.arange(N)[:, None], np.arange(d)[None, :])
    assert np.array_equal(np.sort(idx.ravel()), np.arange(N * d))      # a permutation of the buffer
    return idx


def to_sliced(info, rm):
    out = np.empty(rm.size, dtype=rm.dtype)
    out[sl_index(info).ravel()] = rm.ravel()
    return out


def from_sliced(info, sl):
    N, d = info.n_users + info.n_items, info.dim
    return sl.ravel()[sl_index(info)].reshape(N, d).copy()


# ---------------------------------------------------------------------------------------------- epilogues of rk_spmm_lds
def addend_separate(w, add):
    """v = fl(fl(acc * dinv) + add): scale and add rounded separately"""
    return w.y0 + add


def addend_fused(w, add):
    """v = fl(acc * dinv + add): one FMA (the product of two fp32 is exact in float64; the float64 sum is rounded once more to
    fp32 -- a double rounding that can differ from the FMA in rare ties, which is why this form is only REPORTED)"""
    return (w.acc.astype(np.float64) * w.dinv.astype(np.float64)[:, None] + add.astype(np.float64)).astype(np.float32)


def addend_budget(w, add):
    """(exact value in float64, budget): two roundings, u (|acc dinv| + |acc dinv + add|), whichever way they fall"""
    prod = w.acc.astype(np.float64) * w.dinv.astype(np.float64)[:, None]
    v = prod + add.astype(np.float64)
    return v, U32 * (np.abs(prod) + np.abs(v))


def running_sum(sum_in, v, scale):
    """sum_out = fl(fl(sum_in + v) * scale): (a + b) * c cannot contract"""
    return (sum_in + v) * np.float32(scale)


def running_sum_budget(sum_in, v_bound, v_exact, scale):
    """y not requested: the addend budget carried through, plus 2u (|sum_in| + |v|) |scale| for the sum's own two roundings"""
    return (v_bound + 2 * U32 * (np.abs(sum_in.astype(np.float64)) + np.abs(v_exact))) * abs(float(np.float32(scale)))


def adam(p, m, v, g, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """row-major p / m / v after one torch.optim.Adam step with gradient g, by the oracle (every operation rounded on its own,
    like common.h's adam_elem)"""
    from oracle import oracle as orc
    p, m, v = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in (p, m, v))
    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32), m, v, t, lr, b1, b2, eps)
    return p, m, v


# ---------------------------------------------------------------------------------------------- seeded graphs
EDGE_DEGREES = (600, 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2, 0, 511, 512, 513)


def _from_degrees(U, I, deg, rng):
    ptr = np.zeros(U + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rng.choice(I, size=int(k), replace=False)) for k in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, idx


def _transpose(U, I, ptr, idx):
    users = np.repeat(np.arange(U), np.diff(ptr))
    order = np.lexsort((users, idx))
    tptr = np.zeros(I + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(idx, minlength=I))
    return tptr, users[order].astype(np.int32)


def graph(name):
    """(U, I, rowptr, col, val) of the normalised bipartite adjacency of a named seeded graph:
    edge      40 x 600, user degrees cycling through EDGE_DEGREES capped at I: the 8-entry blocks, the two-block rounds, every
              chunk-cap boundary, a row of ten chunks at cap 64 (phase 3's eight-at-a-time loop and its tail), empty rows
    edge_t    its transpose (600 x 40): the other half meets the long rows
    tall      1100 x 40, degrees 0..3 and one full user: more than 1024 rows in ONE block at n_cu = 2 (phase 3's i != tid)
    long1/2/4 8300 / 4200 / 2100 users x 33 items: the users table is more than 8 * 1024 float4 at 1 / 2 / 4 lanes per entry
              (the second trip of the staging loop)
    one       1 x 1;  three  3 x 2 with an empty user"""
    rng = np.random.default_rng(20240611)
    if name in ("edge", "edge_t"):
        U, I = 40, 600
        deg = np.minimum(np.asarray([EDGE_DEGREES[u % len(EDGE_DEGREES)] for u in range(U)]), I)
        ptr, idx = _from_degrees(U, I, deg, rng)
        if name == "edge_t":
            ptr, idx = _transpose(U, I, ptr, idx)
            U, I = I, U
    elif name in ("tall", "long1", "long2", "long4"):
        U, I = dict(tall=(1100, 40), long1=(8300, 33), long2=(4200, 33), long4=(2100, 33))[name]
        deg = rng.integers(0, 4, U)
        deg[0] = I
        ptr, idx = _from_degrees(U, I, deg, rng)
    elif name == "one":
        U, I, ptr, idx = 1, 1, np.asarray([0, 1], dtype=np.int64), np.asarray([0], dtype=np.int32)
    elif name == "three":
        U, I, ptr, idx = 3, 2, np.asarray([0, 2, 2, 3], dtype=np.int64), np.asarray([0, 1, 1], dtype=np.int32)
    else:
        raise KeyError(name)
    return (U, I) + norm_adj_csr(U, I, ptr, idx)


def user_item_csr(name):
    """the same graph as the user -> item CSR (ptr, idx) CsrGraph.from_user_item_csr takes"""
    U, I, rowptr, col, _ = graph(name)
    return U, I, rowptr[: U + 1].astype(np.int64), (col[: rowptr[U]] - U).astype(np.int32)


def _cases():
    """(graph, dim, n_cu, (lpa, lpb), cap): every dispatched pair at the shapes where each loop takes every branch"""
    out = []
    for g in ("edge", "edge_t"):
        for dim in (16, 48):
            for n_cu in (2, 8, 256):
                out += [(g, dim, n_cu, f, 0) for f in FORMS]
        for f in ((1, 1), (2, 2), (4, 4)):
            out += [(g, 16, 8, f, 64), (g, 16, 8, f, 512)]
        out.append((g, 16, 8, (2, 1), 96))
    out += [("tall", 16, 2, (1, 1), 0), ("tall", 48, 2, (1, 1), 128), ("tall", 16, 2, (1, 2), 0)]
    for n_cu in (2, 256):
        out += [("long1", 4, n_cu, (1, 1), 0), ("long2", 8, n_cu, (1, 2), 0), ("long2", 8, n_cu, (2, 2), 0),
                ("long4", 16, n_cu, (2, 4), 0), ("long4", 16, n_cu, (4, 4), 256)]
    for g in ("one", "three"):
        out += [(g, 16, 8, f, 0) for f in FORMS]
    return out


CASES = _cases()


def case_id(c):
    g, dim, n_cu, (a, b), cap = c
    return f"{g}-d{dim}-cu{n_cu}-lp{a}{b}-c{cap}"


_graphs, _plans, _walks = {}, {}, {}


def case_graph(name):
    if name not in _graphs:
        _graphs[name] = graph(name)
    return _graphs[name]


def case_x(c, what="x"):
    """the case's standard_normal operand (x / add / sum_in ...): seeded by the graph, dim and name, the same wherever it is asked for"""
    U, I = case_graph(c[0])[:2]
    seed = [c[1], U, I] + [ord(ch) for ch in what]
    return np.random.default_rng(seed).standard_normal((U + I, c[1])).astype(np.float32)


def case_plan(c):
    """(words, info) of the case's plan through rk_lds_plan_build_host_ex (cached, read-only)"""
    if c not in _plans:
        g, dim, n_cu, form, cap = c
        _plans[c] = build_plan(*case_graph(g), dim, n_cu, FORMS[form], cap)
    return _plans[c]


def case_walk(c):
    """the walk of the case's plan over case_x(c) (cached, read-only; bank-conflict assertions on)"""
    if c not in _walks:
        _walks[c] = walk(case_plan(c)[0], case_x(c))
    return _walks[c]


# ---------------------------------------------------------------------------------------------- the multi-phase queues
def multi_queues(words):
    """The multi-phase launch's work-item queues (plan words at LP_MQ_OFS, csrc/spmm_lds.h)."""
    o = int(words[H["MQ_OFS"]])
    n_queues, n_groups, G = (int(v) for v in words[o: o + 3])
    queues = []
    for q in range(n_queues):
        n_items, first = int(words[o + 4 + 2 * q]), int(words[o + 4 + 2 * q + 1])
        queues.append(words[first * 4: first * 4 + 4 * n_items].reshape(-1, 4))
    members = words[o + 4 + 2 * n_queues: o + 4 + 2 * n_queues + n_groups]
    return n_queues, n_groups, G, queues, members


def check_multi_queues(words, dim, n_phases=3):
    """spmm_lds_multi_kernel's contract with the plan: the queue lists hold every (half, slice, block) workgroup of the
    single-phase table exactly once; a column group (the workgroups that exchange data between consecutive layers) never
    straddles queues and its member count is what the arrival counter waits for; and -- simulated with FEWER resident
    workgroups than the grid, in adversarial order -- handing a queue's items out in phase-major ticket order never leaves a
    running workgroup waiting for an item nobody has taken."""
    n_queues, n_groups, G, queues, members = multi_queues(words)
    S = {0: 1 << int(words[H["LSI"]]), 1: 1 << int(words[H["LSU"]])}
    assert G == max(S.values()) and n_groups == dim // G and 1 <= n_queues <= 8 and n_groups <= 64
    wg = words[int(words[H["WG_OFS"]]): int(words[H["WG_OFS"]]) + 4 * int(words[H["NWG"]])].reshape(-1, 4)
    # the 64-byte workgroup records: table entry + its block descriptor (what the kernels read instead of the header chain)
    rec = words[int(words[H["WGX_OFS"]]): int(words[H["WGX_OFS"]]) + 16 * int(words[H["NWG"]])].reshape(-1, 16)
    assert np.array_equal(rec[:, :3], wg[:, :3])
    for b, (h, s_, rb, _) in enumerate(wg):
        bd = words[int(words[H["BLK_OFS"]]) + ((int(words[H["NBLK0"]]) if h else 0) + int(rb)) * LB["WORDS"]:][: LB["WORDS"]]
        assert np.array_equal(rec[b, 4:12], bd) and int(rec[b, 3]) == int(s_) * S[int(h)] // G
    multi = sorted(int(b) for qv in queues for b, _, _, _ in qv)
    assert multi == list(range(int(words[H["NWG"]])))          # every record exactly once
    count = np.zeros(n_groups, dtype=np.int64)
    for q, qv in enumerate(queues):
        for b, _, _, g in qv:
            assert int(g) == int(rec[int(b), 3]) and int(g) % n_queues == q      # the group of its slice; its home queue
            count[int(g)] += 1
    assert np.array_equal(count, members)
    # ticket-order simulation: R < grid workgroups, each pulls from queue (b % 8) % n_queues; an item of phase p needs all
    # members of its group to have FINISHED phase p - 1.  A workgroup that cannot start spins (keeps its slot).
    rng = np.random.default_rng(dim)
    for resident in (1, 3, max(2, int(words[H["NWG"]]) // 5)):
        head = [0] * n_queues
        arrived = np.zeros(n_groups, dtype=np.int64)
        blocks = list(range(int(words[H["NWG"]])))
        running = {}                                       # block -> (queue, ticket) it holds
        waiting_blocks = blocks[::-1]
        done_items = 0
        total = sum(len(qv) for qv in queues) * n_phases
        for _ in range(50 * total + 100):
            while len(running) < resident and waiting_blocks:      # admit blocks in an arbitrary (reversed) order
                b = waiting_blocks.pop()
                q = (b % 8) % n_queues
                running[b] = (q, head[q]); head[q] += 1
            if not running:
                break
            b = list(running)[int(rng.integers(len(running)))]   # an arbitrary running block makes progress
            q, t = running[b]
            if t >= len(queues[q]) * n_phases:
                del running[b]                                   # queue exhausted: the block exits
                continue
            phase, (_, _, _, g) = t // len(queues[q]), queues[q][t % len(queues[q])]
            if phase > 0 and arrived[int(g)] < members[int(g)] * phase:
                continue                                         # spins
            arrived[int(g)] += 1
            done_items += 1
            running[b] = (q, head[q]); head[q] += 1
        assert done_items == total and not running, (resident, done_items, total)
    # every queue is pulled by at least one workgroup of the launch
    assert {(b & 7) % n_queues for b in range(int(words[H["NWG"]]))} == set(range(n_queues))
