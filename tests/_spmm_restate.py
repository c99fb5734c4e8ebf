"""The row-gather SpMM's schedule (recad_amd/csrc/host/csr_schedule_host.h, host/layout.h) parsed, checked and WALKED in the order
the kernels of recad_amd/csrc/spmm.h add (spmm_segment, gather_round, the packed branch, piece_arrive, spmm_epilogue,
spmm_csr_generic_kernel), plus the case graphs and forms tests/test_spmm_csr_forms_host.py and _gpu.py share.  The layout is
restated here, not imported.  No GPU, no torch.

Schedule words (rk_csr_schedule_words, n_words int32):
    [n_blocks x W] int4 wave descriptors {row, e_begin, e_end, n_segments if the row's leader else 0}; an idle wave is {-1, 0, 0, 0};
                   a packed wave is {first packed row, n rows, longest row, -1}
    int4 header    {n_long, n_slots, dim, n_packed}
    [n_blocks]     int4 workgroup metas {n_pieces, piece index, first slot, counter index}; zeros = whole rows
    [n_packed]     int4 packed short rows {row, e_begin, e_end, 0}
The opaque launch parameter carries n_blocks in its low bits, bit 30 = packed waves present, bits 28-29 = waves per workgroup
(0 = 8, 1 = 4, 2 = 16), bit 27 = long rows present.

The walk, in fp32 (u = 2^-24):
  vector kernel (dim 32 / 64 / 128 / 256), segment: with G = dim / 4 lanes per x row a wave has NG = 64 / G lane groups.  For each
      64-entry chunk of the segment group g takes the chunk's entries t NG + g, t = 0, 1, ... as ONE chain acc = fmaf(val, x[col], acc);
      the chain carries across the chunks of a 128-entry segment.  Then the groups meet in the xor butterfly at group offsets
      1, 2, 4, ... < NG: p[g] = p[g] + p[g ^ o].  (Padding lanes add 0 * x[0]: nothing for finite x[0].)
  row: leader's segment + next + next, in wave order.  Long row: slot 0 + slot 1 + ..., each slot its piece's segment sum.
  packed row: one chain over its entries in CSR order.
  generic kernel (any other dim): one chain per segment in entry order, then segments, then pieces.
  src_filter: each 64-entry chunk is compacted to its hits, in order, and dealt to the groups anew; a packed row keeps its order
      with the misses as zeros (a zero term leaves a chain's bits alone, so the walk skips them).
  dropout: the value of entry e is keep(e) ? fl(val * inv_keep) : 0 (tests/_drop_restate.py), id = e in the forward.
The chains go through the oracle's fmaf chain (orc.score_rows): the kernels ask for the fused multiply-add by name (spmm.h,
f4_fma), so fused = True is the expectation; fused = False rounds the product on its own (plain numpy fp32).  (Written as
`acc += a * x` the contraction had been hipcc's choice per inlined copy: at dim 32 the 4-deep gather rounds rounded their
products and the 8-deep ones fused them, at dim 64 the other way round -- found by the first run of
test_no_addend_equals_the_walk_bit_for_bit[d32-w4-s64]; no table of instantiations could describe that.)"""
import ctypes as C
import functools

import numpy as np

from . import _drop_restate as DR

U32 = 2.0 ** -24
PACKED_FLAG, LONG_FLAG, WAVES_SHIFT, WAVES_MASK = 1 << 30, 1 << 27, 28, 3 << 28
VEC_DIMS = (32, 64, 128, 256)
RK_EINVAL = -22

# Instantiations that match only the UNFUSED walk, never a wider tolerance: (dim, waves, packed, drop, filt) -> False.
# Empty: with the fused multiply-add asked for by name every instantiation reproduces the fused walk.
UNFUSED = {}


def sched_waves(n_blocks_param):
    return {1: 4, 2: 16}.get((n_blocks_param & WAVES_MASK) >> WAVES_SHIFT, 8)


def plain_blocks(n_blocks_param):
    return n_blocks_param & ~(PACKED_FLAG | WAVES_MASK | LONG_FLAG)


# ---------------------------------------------------------------------------------------------- building
def build_handle(rowptr, class_split, dim, form=None):
    """-> (rc, handle, n_blocks, n_words, scratch_words); form None = rk_csr_schedule_build_host, else (waves, seg_nnz, pack) through
    rk_csr_schedule_build_host_ex.  The caller destroys the handle."""
    from recad_amd import _lib
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    sched, nb, nw, sw = C.c_void_p(), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    tail = (C.byref(sched), C.byref(nb), C.byref(nw), C.byref(sw))
    if form is None:
        rc = _lib.lib().rk_csr_schedule_build_host(len(rp) - 1, rp.ctypes.data_as(C.c_void_p), class_split, dim, *tail)
    else:
        rc = _lib.lib().rk_csr_schedule_build_host_ex(len(rp) - 1, rp.ctypes.data_as(C.c_void_p), class_split, dim, *form, *tail)
    return rc, (sched if rc == 0 else None), nb.value, nw.value, sw.value


def handle_words(handle, n_words):
    from recad_amd import _lib
    w = np.zeros(n_words, dtype=np.int32)
    _lib.check(_lib.lib().rk_csr_schedule_words(handle, w.ctypes.data_as(C.c_void_p)), "rk_csr_schedule_words")
    return w


def build(rowptr, class_split, dim, form=None):
    """-> (words, n_blocks, scratch_words) of a schedule that must build"""
    from recad_amd import _lib
    rc, h, nb, nw, sw = build_handle(rowptr, class_split, dim, form)
    assert rc == 0, _lib.lib().rk_last_error()
    try:
        return handle_words(h, nw), nb, sw
    finally:
        _lib.lib().rk_csr_schedule_destroy(h)


class Sched:
    """the parsed words"""

    def __init__(self, words, n_blocks_param):
        self.param = int(n_blocks_param)
        self.W, self.nb = sched_waves(self.param), plain_blocks(self.param)
        o = self.nb * self.W * 4
        assert len(words) >= o + 4 + 4 * self.nb, "schedule words too short for their own block count"
        self.desc = np.asarray(words[:o]).reshape(self.nb, self.W, 4)
        self.n_long, self.n_slots, self.dim, self.n_packed = (int(a) for a in words[o:o + 4])
        self.meta = np.asarray(words[o + 4:o + 4 + 4 * self.nb]).reshape(self.nb, 4)
        rest = np.asarray(words[o + 4 + 4 * self.nb:])
        assert rest.size == 4 * self.n_packed, "the packed-row table does not have the header's n_packed rows"
        self.packed = rest.reshape(self.n_packed, 4)


def check_structure(s, rowptr, dim, seg_nnz, class_split, scratch_words):
    """The structural contract of a schedule (module docstring of the issue): raises AssertionError naming what is broken."""
    rp = np.asarray(rowptr, dtype=np.int64)
    n_rows, nnz = len(rp) - 1, int(rp[-1])
    assert s.dim == dim
    assert bool(s.param & PACKED_FLAG) == (s.n_packed > 0) and bool(s.param & LONG_FLAG) == (s.n_long > 0)
    assert s.W in (4, 8, 16) and seg_nnz in (64, 128)
    cover = np.zeros(nnz, dtype=np.int32)
    seen = np.zeros(n_rows, dtype=np.int32)           # rows finished by a whole-row leader or a packed lane group
    packed_used = np.zeros(s.n_packed, dtype=np.int32)
    pieces = {}                                        # counter index -> list of (piece index, n_pieces, first slot, row, e_begin, e_end)
    block_class = np.zeros(s.nb, dtype=np.int32)
    G = dim // 4
    for b in range(s.nb):
        d, m = s.desc[b], s.meta[b]
        rows_here = []
        w = 0
        n_leaders = 0
        while w < s.W:
            r, eb, ee, k = (int(a) for a in d[w])
            if k < 0:                                  # packed wave
                assert dim in (32, 64, 128), "a packed wave at a dim that cannot pack"
                first, cnt, longest = r, eb, ee
                assert 1 <= cnt <= 256 // dim and 0 <= first and first + cnt <= s.n_packed
                lens = []
                for q in range(first, first + cnt):
                    pr, pb, pe, pz = (int(a) for a in s.packed[q])
                    assert 0 <= pr < n_rows and pb == rp[pr] and pe == rp[pr + 1] and pz == 0, "a packed row is not its whole CSR row"
                    assert pe - pb <= G, "a packed row has more than dim / 4 nonzeros"
                    cover[pb:pe] += 1
                    seen[pr] += 1
                    packed_used[q] += 1
                    lens.append(pe - pb)
                    rows_here.append(pr)
                assert longest == max(lens), "a packed wave's ds.z is not its longest row"
                assert m[0] == 0, "a packed wave inside a long row's piece"
                w += 1
                continue
            if r < 0:
                assert (r, eb, ee, k) == (-1, 0, 0, 0), "an idle wave is {-1, 0, 0, 0}"
                w += 1
                continue
            assert k >= 1, "a segment wave that no leader counts"
            assert 0 <= r < n_rows and w + k <= s.W
            n_leaders += 1
            rows_here.append(r)
            prev = eb
            for j in range(k):
                rj, ebj, eej, kj = (int(a) for a in d[w + j])
                assert rj == r and (kj == k if j == 0 else kj == 0), "a row's segments: consecutive waves, the leader carries the count, the others 0"
                assert ebj == prev and ebj <= eej and eej - ebj <= seg_nnz and rp[r] <= ebj and eej <= rp[r + 1]
                assert j == k - 1 or eej - ebj == seg_nnz, "only a row's last segment may be short"
                cover[ebj:eej] += 1
                prev = eej
            if m[0] > 0:
                pieces.setdefault(int(m[3]), []).append((int(m[1]), int(m[0]), int(m[2]), r, eb, prev))
            else:
                assert eb == rp[r] and prev == rp[r + 1], "a whole row's segments do not span the row"
                seen[r] += 1
            w += k
        if m[0] > 0:
            assert n_leaders == 1 and int(d[0][3]) >= 1, "a long row's piece is one leader at wave 0"
        else:
            assert not m.any(), "the meta of a workgroup of whole rows is zeros"
        assert rows_here, "a workgroup without work"
        cls = {int(class_split > 0 and r >= class_split) for r in rows_here}
        assert len(cls) == 1, "a workgroup mixes the two classes"
        block_class[b] = cls.pop()
    assert (packed_used == 1).all()
    slots = np.zeros(s.n_slots, dtype=np.int32)
    assert sorted(pieces) == list(range(s.n_long)), "counter indices are 0 .. n_long - 1, one per long row"
    for ci, ps in pieces.items():
        ps.sort()
        n_p, slot0, r = ps[0][1], ps[0][2], ps[0][3]
        assert [p[0] for p in ps] == list(range(n_p)) and n_p >= 2, "piece indices 0 .. np - 1"
        assert all(p[1] == n_p and p[2] == slot0 and p[3] == r for p in ps)
        assert ps[0][4] == rp[r] and ps[-1][5] == rp[r + 1] and all(a[5] == b_[4] for a, b_ in zip(ps, ps[1:])), "the pieces do not tile the row"
        assert all(p[5] - p[4] == s.W * seg_nnz for p in ps[:-1]), "only a long row's last piece may be short"
        assert 0 <= slot0 and slot0 + n_p <= s.n_slots
        slots[slot0:slot0 + n_p] += 1
        seen[r] += 1
    assert (slots == 1).all(), "slots are not used exactly once"
    assert (seen == 1).all(), "a row is finished by no wave, or by two"
    assert (cover == 1).all(), "a stored entry lies in no segment, or in two"
    want_scratch = ((s.n_long + 3) & ~3) + s.n_slots * dim if s.n_long else 0
    assert scratch_words == want_scratch
    nb1 = int(block_class.sum())
    nb0 = s.nb - nb1
    i0 = i1 = 0
    for b in range(s.nb):                               # 4 : 4 per group of 8 while both lists last
        want1 = (b % 8) >= 4
        if want1 and i1 >= nb1:
            want1 = False
        if not want1 and i0 >= nb0:
            want1 = True
        assert block_class[b] == int(want1), ("class interleave", b)
        i0, i1 = i0 + (not want1), i1 + want1


# ---------------------------------------------------------------------------------------------- the walk
def chain(vals, xrows, fused=True):
    """acc[c] = fmaf(vals[k], xrows[k, c], acc[c]) over k from +0.0 (fused) or fl(acc + fl(v x)) -> fp32 [d]"""
    K = len(vals)
    if K == 0:
        return np.zeros(xrows.shape[1], dtype=np.float32)
    if fused:
        from oracle import oracle as orc
        return orc.score_rows(np.ascontiguousarray(vals, dtype=np.float32)[None, :], np.ascontiguousarray(xrows.T, dtype=np.float32))[0]
    acc = np.zeros(xrows.shape[1], dtype=np.float32)
    for k in range(K):
        acc = acc + np.float32(vals[k]) * xrows[k]
    return acc


WRONG = ("pieces_reversed", "segment_dropped", "groups_linear", "hits_not_compacted", "packed_reversed")


def _segment(col, val, x, eb, ee, dim, fused, hit, wrong):
    """one wave's segment [eb, ee) -> its fp32 partial sum [dim]"""
    if dim not in VEC_DIMS:
        return chain(val[eb:ee], x[col[eb:ee]], fused)
    NG = 64 // (dim // 4)
    lists = [[] for _ in range(NG)]
    for base in range(eb, ee, 64):
        ents = np.arange(base, min(base + 64, ee))
        if hit is not None:
            if wrong == "hits_not_compacted":
                for g in range(NG):
                    mine = ents[g::NG]
                    lists[g].append(mine[hit[col[mine]]])
                continue
            ents = ents[hit[col[ents]]]
        for g in range(NG):
            lists[g].append(ents[g::NG])
    p = []
    for g in range(NG):
        e = np.concatenate(lists[g]) if lists[g] else np.zeros(0, dtype=np.int64)
        p.append(chain(val[e], x[col[e]], fused))
    if wrong == "groups_linear":
        acc = p[0]
        for g in range(1, NG):
            acc = acc + p[g]
        return acc
    o = 1
    while o < NG:
        p = [p[g] + p[g ^ o] for g in range(NG)]
        o <<= 1
    return p[0]


def walk(s, rowptr, col, val, x, fused=True, hit=None, wrong=None):
    """A x in the kernel's own order -> fp32 [n_rows, dim].  hit: bool over x's rows (src_filter; vector kernels only, the generic
    kernel ignores it like spmm_launch does).  wrong: one of WRONG, a deliberately wrong order (the discrimination checks)."""
    rp = np.asarray(rowptr, dtype=np.int64)
    col, val, x = np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float32), np.asarray(x, dtype=np.float32)
    dim = x.shape[1]
    assert dim == s.dim
    if dim not in VEC_DIMS:
        hit = None
    y = np.zeros((len(rp) - 1, dim), dtype=np.float32)
    slots = {}
    for b in range(s.nb):
        d, m = s.desc[b], s.meta[b]
        w = 0
        while w < s.W:
            r, eb, ee, k = (int(a) for a in d[w])
            if k < 0:
                for q in range(r, r + eb):
                    pr, pb, pe, _ = (int(a) for a in s.packed[q])
                    e = np.arange(pb, pe)
                    if hit is not None:
                        e = e[hit[col[e]]]
                    if wrong == "packed_reversed":
                        e = e[::-1]
                    y[pr] = chain(val[e], x[col[e]], fused)
                w += 1
                continue
            if r < 0 or k == 0:
                w += 1
                continue
            acc = None
            for j in range(k):
                if wrong == "segment_dropped" and j == 1:
                    continue
                part = _segment(col, val, x, int(d[w + j][1]), int(d[w + j][2]), dim, fused, hit, wrong)
                acc = part if acc is None else acc + part
            if m[0] > 0:
                slots.setdefault((r, int(m[0])), {})[int(m[1])] = acc
            else:
                y[r] = acc
            w += k
    for (r, n_p), ps in slots.items():
        order = range(n_p - 1, -1, -1) if wrong == "pieces_reversed" else range(n_p)
        acc = None
        for q in order:
            acc = ps[q] if acc is None else acc + ps[q]
        y[r] = acc
    return y


def drop_values(val, seed_step, keep_prob):
    """the values a dropout launch multiplies by: entry e kept iff its 24-bit uniform < (double)(float)keep_prob * 2^24, and then
    fl(val * fl(1 / keep_prob)); id = e (the forward)"""
    kp = np.float32(keep_prob)
    thresh = int(float(kp) * 16777216.0)
    with np.errstate(over="ignore"):
        ids = np.arange(len(val), dtype=np.uint64) * np.uint64(0xD1342543DE82EF95)
        keep = (DR._mix64(np.uint64(seed_step) ^ ids) >> np.uint64(40)) < np.uint64(thresh)
    inv = np.float32(1.0) / kp
    return np.where(keep, np.asarray(val, dtype=np.float32) * inv, np.float32(0.0)).astype(np.float32), keep


def exact(rowptr, col, val, x, hit=None):
    """(A x in float64, sum |terms|) per element, hit = the filter"""
    rp = np.asarray(rowptr, dtype=np.int64)
    n, d = len(rp) - 1, x.shape[1]
    v, mag = np.zeros((n, d)), np.zeros((n, d))
    for r in range(n):
        e = np.arange(rp[r], rp[r + 1])
        if hit is not None:
            e = e[hit[np.asarray(col)[e]]]
        if len(e):
            prod = np.asarray(val, dtype=np.float64)[e, None] * np.asarray(x, dtype=np.float64)[np.asarray(col)[e]]
            v[r], mag[r] = prod.sum(0), np.abs(prod).sum(0)
    return v, mag


def running_sum(sum_in, v, scale):
    """sum_out = fl(fl(sum_in + v) * scale): an add, then a multiply -- nothing to fuse"""
    return (np.asarray(sum_in, dtype=np.float32) + np.asarray(v, dtype=np.float32)) * np.float32(scale)


def adam(p, m, v, g, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    from oracle import oracle as orc
    p, m, v = (np.ascontiguousarray(a, dtype=np.float32).copy() for a in (p, m, v))
    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32), m, v, t, lr, b1, b2, eps)
    return p, m, v


def bits_of(hit):
    """bool over rows -> the uint32 bitmap words the kernels test"""
    n = len(hit)
    padded = np.zeros(((n + 31) // 32) * 32, dtype=np.uint64)
    padded[:n] = hit
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- cases
N_BODY = 280


def case_degrees(dim, W, seg):
    """the row lengths of the case graph of (dim, W, seg): see the module docstring of tests/test_spmm_csr_forms_gpu.py"""
    G = max(dim // 4, 1)
    special = [0, 0, 1, G - 1, G, G + 1, seg - 1, seg, seg + 1, 2 * seg + 1, W * seg, W * seg + 1, 8 * W * seg + 1, 9 * W * seg + 5]
    rng = np.random.default_rng([dim, W, seg])
    body = rng.poisson(max(G, 3), N_BODY)
    deg = np.concatenate([np.asarray(special, dtype=np.int64), body])
    return deg[rng.permutation(len(deg))], special


def _normal(rng, *shape):
    """normal fp32 away from zero: no subnormal input, no subnormal product"""
    a = rng.standard_normal(shape).astype(np.float32)
    return np.where(np.abs(a) < 1e-3, np.float32(1e-3), a).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_graph(dim, W, seg):
    """(rowptr int32, col int32, val fp32, x_rows): x is taller than the graph -- as many rows as the longest row has columns"""
    deg, _ = case_degrees(dim, W, seg)
    x_rows = int(deg.max())
    rng = np.random.default_rng([7, dim, W, seg])
    rowptr = np.zeros(len(deg) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(deg)
    col = np.concatenate([np.sort(rng.choice(x_rows, size=int(k), replace=False)) for k in deg]).astype(np.int32)
    val = _normal(rng, len(col)) * np.float32(0.25)
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val, x_rows


@functools.lru_cache(maxsize=None)
def case_x(dim, W, seg, which="x"):
    rowptr, _, _, x_rows = case_graph(dim, W, seg)
    rng = np.random.default_rng([11, dim, W, seg, {"x": 0, "add": 1, "sum_in": 2}[which]])
    a = _normal(rng, x_rows if which == "x" else len(rowptr) - 1, dim)
    a.setflags(write=False)
    return a


# (dim, W, seg, pack, split): pack -1 = off, 1 = every short row; split: class_split in the middle
VEC_FORMS = tuple((d, W, seg, -1, 0) for d in VEC_DIMS for W in (4, 8, 16) for seg in (64, 128))
PACK_FORMS = tuple((d, W, 64, 1, 0) for d in (32, 64, 128) for W in (4, 8, 16)) + ((64, 4, 128, 1, 0), (32, 8, 128, 1, 0))
GEN_FORMS = tuple((d, W, 64, -1, 0) for d in (48, 100, 7) for W in (4, 8, 16)) + ((100, 4, 128, -1, 0),)
SPLIT_FORMS = ((64, 4, 64, -1, 1), (64, 8, 64, 1, 1), (128, 16, 128, -1, 1), (48, 8, 64, -1, 1), (32, 4, 64, 1, 1))
FORMS = VEC_FORMS + PACK_FORMS + GEN_FORMS + SPLIT_FORMS


def form_id(f):
    d, W, seg, pack, split = f
    return f"d{d}-w{W}-s{seg}" + ("-pack" if pack == 1 else "") + ("-split" if split else "")


def form_split(f):
    return (len(case_graph(*f[:3])[0]) - 1) // 2 if f[4] else 0


@functools.lru_cache(maxsize=None)
def form_sched(f):
    """(words, n_blocks, scratch_words, Sched) of the form's schedule through rk_csr_schedule_build_host_ex (cached, read-only)"""
    d, W, seg, pack, _ = f
    words, nb, sw = build(case_graph(d, W, seg)[0], form_split(f), d, (W, seg, pack))
    words.setflags(write=False)
    return words, nb, sw, Sched(words, nb)


@functools.lru_cache(maxsize=None)
def form_walk(f, fused=True):
    rowptr, col, val, _ = case_graph(*f[:3])
    y = walk(form_sched(f)[3], rowptr, col, val, case_x(*f[:3]), fused=fused)
    y.setflags(write=False)
    return y


def case_hits(f, which):
    """the source bitmaps of the filter cases as bool over x's rows: ~3 %, ~50 %, the 64 columns of one whole chunk of the longest
    row (that chunk hits with all 64 lanes; nearly every other chunk with none), one column, all, none"""
    rowptr, col, _, x_rows = case_graph(*f[:3])
    rng = np.random.default_rng([13, f[0], f[1], f[2]])
    if which == "p03":
        return rng.random(x_rows) < 0.03
    if which == "p50":
        return rng.random(x_rows) < 0.5
    hit = np.zeros(x_rows, dtype=bool)
    if which == "chunk":
        r = int(np.argmax(np.diff(rowptr)))
        hit[col[rowptr[r] + 64:rowptr[r] + 128]] = True
    elif which == "one":
        hit[x_rows // 3] = True
    elif which == "ones":
        hit[:] = True
    else:
        assert which == "zeros"
    return hit
