"""Numpy restatement of the scoring + top-K selection of recad_amd/csrc/score_topk.hip and score_panel.h, the case tables that
tests/test_select_host.py (CPU) and tests/test_score_select_forms_gpu.py (MI355X) both run, and the dispatch of the two entry
points written down as DATA, each entry with the source line it was read from (the host test checks that the FILE still says so:
it searches for the text, so an edit above a line moves nothing; the numbers are where to look, as of this writing).

The reference of a selection is select_row(): keys by score_key() on uint32, the lists ordered by (key desc, id asc) over the
RANKABLE items -- unseen and key > 0 -- and a target's rank counted over the same items.  What is not rankable: a seen item, -inf
and negative NaNs (key 0).  A positive NaN ranks above +inf.  On finite rows this is orc.topk_row bit for bit, except that a -0.0
comes back from the kernels' lists as +0.0 (key_score inverts the folded key), which the host test states where it compares.

A SEEN target (read from oracle.topk_row and the three selection kernels, which agree): its score is reported as computed (the
raw entry of the matrix, -0.0 and signalling NaNs included: it is a copy, not a key), and its rank is counted as if it were
rankable -- #(key > key_t) + #(key == key_t, id < t) over the rankable items other than itself.  A target whose own key is 0 (its
score is -inf or a negative NaN) ranks behind every rankable item: rank = their number (the kernels' `k != 0u` in
topk_rows_kernel, the kKeyValid - 1 stand-in in topk_wave_kernel)."""
import functools

import numpy as np

U32 = np.uint32
NEG_INF_BITS = U32(0xff800000)
SCORE_TOPK = "recad_amd/csrc/score_topk.hip"
SCORE_PANEL = "recad_amd/csrc/score_panel.h"
MAX_K, MAX_TARGETS, IN_PASS_TARGETS, PANEL_MAX_T = 256, 256, 4, 4
HEADER_SAYS = "The panel path requires finite tables"       # include/recad_hip.h, at rk_score_topk


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


# ------------------------------------------------------------------------------------------------------------------ keys
def score_key(scores):
    """score_panel.h score_key on uint32 bit patterns: `s + 0.0f` (folds -0.0 onto +0.0, quiets a signalling NaN: sets the top
    mantissa bit, sign and payload kept), the monotone map (negative: all bits flipped, positive: sign bit set), and the clamp of
    everything at or below -inf's image 0x007fffff (-inf itself and the negative NaNs) to 0 = excluded."""
    u = bits(scores).copy()
    u[u == U32(0x80000000)] = U32(0)
    nan = ((u & U32(0x7f800000)) == U32(0x7f800000)) & ((u & U32(0x007fffff)) != 0)
    u[nan] |= U32(0x00400000)
    k = np.where(u >> U32(31) != 0, ~u, u | U32(0x80000000)).astype(U32)
    k[k <= U32(0x007fffff)] = U32(0)
    return k


def key_score(keys):
    """score_panel.h key_score: the float (as bits) of a key; exact inverse for every finite score, +inf and the quieted NaNs"""
    k = np.ascontiguousarray(keys, dtype=U32)
    return np.where(k & U32(0x80000000) != 0, k ^ U32(0x80000000), ~k).astype(U32)


def select_row(scores, seen, K, targets, fault=None):
    """-> (top_ids int32[K], top_scores float32[K], target_score float32[T], target_rank int32[T]) of one row.
    fault: one of FAULTS, a selection that is wrong in one planted way (tests/test_select_host.py)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n = len(scores)
    ids = np.arange(n, dtype=np.int64)
    raw = score_key(scores)
    if fault == "neg_zero_below":
        raw = np.where(bits(scores) == U32(0x80000000), U32(0x7fffffff), raw).astype(U32)      # the unfolded image of -0.0
    key = raw.copy()
    key[np.asarray(seen, dtype=np.int64)] = 0
    rankable = key > 0
    if fault == "drop_64q":
        rankable = rankable & ~((ids % 64 == 0) & (ids > 0))
    cand = ids[rankable]
    tie = -cand if fault == "ties_higher_id" else cand
    order = cand[np.lexsort((tie, -key[cand].astype(np.int64)))][:K]
    top_ids = np.full(K, 7 if fault == "no_padding" else -1, dtype=np.int32)
    top_bits = np.full(K, U32(0x40e00000) if fault == "no_padding" else NEG_INF_BITS, dtype=U32)
    top_ids[:len(order)] = order
    top_bits[:len(order)] = key_score(key[order])
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    t_score = scores[targets] if len(targets) else np.zeros(0, dtype=np.float32)
    t_rank = np.zeros(len(targets), dtype=np.int32)
    for j, t in enumerate(targets):
        kt = raw[t]
        others = (key > 0) if fault != "seen_in_rank" else (raw > 0)
        others = others & (ids != t)
        k = key if fault != "seen_in_rank" else raw
        above = k > kt
        if fault == "rank_ge":
            above = k >= kt
        t_rank[j] = int(np.count_nonzero(others & (above | ((k == kt) & (ids < t)))))
    return top_ids, top_bits.view(np.float32), t_score.copy(), t_rank


FAULTS = ("ties_higher_id", "rank_ge", "seen_in_rank", "neg_zero_below", "drop_64q", "no_padding")


def same_row(got, ref):
    """ids, score BITS, target score bits and ranks"""
    return (np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(bits(got[2]), bits(ref[2]))
            and np.array_equal(got[3], ref[3]))


def fold_zero(a):
    """-0.0 -> +0.0, every other float unchanged: what a list's score has gone through (key_score(score_key(s)))"""
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(a, dtype=np.float32) + np.float32(0.0)


# ---------------------------------------------------------------------------------------------------------------- scores
def score_rows(urows, itab, ub_rows=None, ib=None, mean=0.0):
    """The float32 fmaf chain in k order (orc.score_rows without biases: one rounding per k, from 0.f) followed by the bias order
    of every scoring form, ((dot + ub) + ib) + mean, each sum rounded to float32.  Asserted against orc.score_rows with biases
    (tests/test_select_host.py) -- and that the other associations give other bits on the bias case."""
    from oracle import oracle as orc
    dot = orc.score_rows(urows, itab)
    if ib is None:
        return dot
    with np.errstate(invalid="ignore", over="ignore"):
        s = dot + np.asarray(ub_rows, dtype=np.float32)[:, None]
        s = s + np.asarray(ib, dtype=np.float32)[None, :]
        return (s + np.float32(mean)).astype(np.float32)


# ------------------------------------------------------------------------------------------- the dispatch, read from the source
# rk_topk_rows: n_items -> the selection form.  (first I, last I, form, NQ, file, line, what the line says)
SELECT_FORMS = (
    (1, 1024, "wave", 16, SCORE_TOPK, 674, "if (nq <= 16) RK_TOPK_WAVE(16);"),
    (1025, 2048, "wave", 32, SCORE_TOPK, 675, "else if (nq <= 32) RK_TOPK_WAVE(32);"),
    (2049, 3072, "wave", 48, SCORE_TOPK, 676, "else if (nq <= 48) RK_TOPK_WAVE(48);"),
    (3073, 3712, "wave", 58, SCORE_TOPK, 677, "else if (nq <= 58) RK_TOPK_WAVE(58);"),
    (3713, 4096, "wave", 64, SCORE_TOPK, 678, "else if (nq <= 64) RK_TOPK_WAVE(64);"),
    (4097, 5120, "wave", 80, SCORE_TOPK, 679, "else if (nq <= 80) RK_TOPK_WAVE(80);"),
    (5121, 5632, "wave", 88, SCORE_TOPK, 680, "else if (nq <= 88) RK_TOPK_WAVE(88);"),
    (5633, 6144, "wave", 96, SCORE_TOPK, 681, "else RK_TOPK_WAVE(96);"),
    (6145, 10240, "lds_rows", 0, SCORE_TOPK, 692, "if (row_bytes <= lds_row_max) {"),
    (10241, 2 ** 31 - 1, "l2_rows", 0, SCORE_TOPK, 704, "hipLaunchKernelGGL((topk_rows_kernel<false>)"),
)
SOURCE_FACTS = (    # the constants the table above leans on
    (SCORE_TOPK, 667, "if (!no_wave && n_items <= 96 * 64) {"),
    (SCORE_TOPK, 668, "const int nq = (n_items + 63) / 64;"),
    (SCORE_TOPK, 691, '(size_t)RK_TUNE_INT("RK_TOPK_LDS_KB", 40) * 1024;'),
    (SCORE_TOPK, 16, "kInPassTargets = 4;"),
    (SCORE_TOPK, 632, "if (n_sel <= 64) rank_all("),
    (SCORE_TOPK, 633, "else if (n_sel <= 128) rank_all("),
    (SCORE_TOPK, 721, "return ((long long)n_items + 31) & ~31LL;"),
    (SCORE_TOPK, 752, "pl.panel_ntw = ntw ? ntw : pan_ntw(n_items);"),
    (SCORE_TOPK, 753, "pl.panel_rows = pl.panel_ntw == 8 ? 16 : (rows ? rows : pan_rows(nb, n_items, dim, n_targets));"),
    (SCORE_PANEL, 924, "return d <= 32 ? 2 : d <= 64 ? 4 : d <= 128 ? 8 : 16;"),
    (SCORE_PANEL, 930, "return (long long)n_items * 16 * pan_dc(d) + 4;"),
    (SCORE_PANEL, 936, "if (n_targets > 1) return 16;"),
    (SCORE_PANEL, 937, "return nb >= 8192 && (d > 64 || n_items >= 65536) ? 32 : 16;"),
    (SCORE_PANEL, 941, "return n_items <= 1024 ? 8 : 15;"),
    (SCORE_PANEL, 961, "return a.n_targets <= 1 ? pan_launch_one<NTW, DC, 1, RB>(a, s) : pan_launch_one<NTW, DC, kPanMaxT, RB>(a, s);"),
    (SCORE_PANEL, 994, "if (ntw == 8) return pan_launch_dc<8, 1>(a, s);"),
    (SCORE_PANEL, 995, "return rows == 32 ? pan_launch_dc<15, 2>(a, s) : pan_launch_dc<15, 1>(a, s);"),
)
WAVE_NQ = tuple(f[3] for f in SELECT_FORMS if f[2] == "wave")
LDS_ROW_MAX_ITEMS = 10240
# rk_score_topk, panel path: (dim, n_targets, request) -> <NTW, DC, NTG, RB>
PANEL_DC = ((32, 2), (64, 4), (128, 8), (256, 16))                                      # score_panel.h:924  pan_dc
PANEL_NTG = ((1, 1), (PANEL_MAX_T, 4))                                                  # score_panel.h:961  pan_launch_tg
PANEL_SHAPES = ((15, 1), (15, 2), (8, 1))                                               # score_panel.h:994-995 (NTW, RB)
PANEL_INSTANTIATIONS = tuple((ntw, dc, ntg, rb) for ntw, rb in PANEL_SHAPES for _, dc in PANEL_DC for _, ntg in PANEL_NTG)
PANEL_REQUESTS = {(15, 1): {"path": "panel", "panel_rows": 16, "panel_ntw": 15}, (15, 2): {"path": "panel", "panel_rows": 32, "panel_ntw": 15},
                  (8, 1): {"path": "panel", "panel_rows": 16, "panel_ntw": 8}}


def select_form(n_items):
    for lo, hi, form, nq, *_ in SELECT_FORMS:
        if lo <= n_items <= hi:
            return form, nq
    raise ValueError(n_items)


def pan_dc(d):
    return next(dc for top, dc in PANEL_DC if d <= top)


def panel_plan(nb, n_items, d, n_targets, request):
    """rk_score_topk_plan's panel branch (score_topk.hip:750-755): -> (panel_rows, panel_ntw, scratch_floats)"""
    ntw = request.get("panel_ntw", 0) or (8 if n_items <= 1024 else 15)
    rows = request.get("panel_rows", 0) or (16 if n_targets > 1 else 32 if nb >= 8192 and (d > 64 or n_items >= 65536) else 16)
    return (16 if ntw == 8 else rows), ntw, n_items * 16 * pan_dc(d) + 4


def panel_instantiation(nb, n_items, d, n_targets, request):
    rows, ntw, _ = panel_plan(nb, n_items, d, n_targets, request)
    return ntw, pan_dc(d), next(g for top, g in PANEL_NTG if n_targets <= top), rows // 16


def score_ld(n_items):
    return (n_items + 31) // 32 * 32                                                    # score_topk.hip:721


# ------------------------------------------------------------------------------------------------ selection cases (rk_topk_rows)
EDGE_I = (1, 1024, 1025, 2048, 2049, 3072, 3073, 3712, 3713, 4096, 4097, 5120, 5121, 5632, 5633, 6144, 6145, 10240, 10241)
FORM_I = (3702, 8000, 10241)               # one wave-kernel, one LDS-row and one L2-row catalogue for the K and target axes
K_AXIS = (1, 63, 64, 65, 127, 128, 129, 255, 256)
T_AXIS = (0, 1, 4, 5, 64, 256)
ROW_KINDS = {5: ("random", "const", "tie64", "few_unseen", "all_seen"), 4: ("tie64", "zeros", "random", "const"),
             3: ("const", "tie64", "random"), 1: ("tie64",)}
N_USERS_EXTRA = 3                          # the user table is this much larger than the block


def _seed(*parts):
    return int(np.random.SeedSequence([int(p) for p in parts]).generate_state(1)[0])


def _row(kind, n, K, rng):
    """-> (scores float32[n], seen int32[] ascending)"""
    scores = rng.standard_normal(n, dtype=np.float32)
    seen = np.sort(rng.choice(n, size=int(rng.integers(0, min(n, 40) + 1)), replace=False))
    if kind == "const":
        scores[:] = 3.0
    elif kind == "zeros":
        scores = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30], dtype=np.float32), size=n)
    elif kind == "tie64":
        # the row's largest value on both sides of its first and its last 64-item boundary, and nowhere seen
        top = np.float32(9.0)
        for q in {1, (n - 1) // 64}:
            for i in (64 * q - 1, 64 * q, 64 * q + 1):
                if 0 <= i < n and q > 0:
                    scores[i] = top
        seen = seen[scores[seen] != top]
    elif kind == "few_unseen":
        unseen = np.sort(rng.choice(n, size=min(n, max(K - 1, 0)), replace=False))
        seen = np.setdiff1d(np.arange(n), unseen)
    elif kind == "all_seen":
        seen = np.arange(n)
    return np.ascontiguousarray(scores, dtype=np.float32), seen.astype(np.int32)


def _targets(n, T, rng, seen_item):
    """a seen target first (item `seen_item` is put into the seen list of every other user), then 0, I - 1, a duplicate, the rest drawn"""
    fixed = [seen_item, 0, n - 1, seen_item, n // 2]
    t = fixed[:T] + [int(x) for x in rng.integers(0, n, size=max(T - len(fixed), 0))]
    return np.asarray(t, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def sel_case(n, nb, K, T):
    """One rk_topk_rows call: scores [nb, n], a user table of nb + 3 seen lists, user_ids a permutation of it with one repeat."""
    rng = np.random.default_rng(_seed(n, nb, K, T))
    kinds = ROW_KINDS[nb]
    nu = nb + N_USERS_EXTRA
    user_ids = rng.permutation(nu)[:nb].astype(np.int32)
    if nb > 1:
        user_ids[1] = user_ids[0]                       # the repeat
    seen_item = 7 % n
    seen_lists = [np.zeros(0, np.int32)] * nu
    scores = np.empty((nb, n), dtype=np.float32)
    for b in range(nb):
        s, seen = _row(kinds[b], n, K, rng)
        if nb > 1 and b == 1:                           # the repeated user: the list of row 0, the kind's scores
            seen = seen_lists[int(user_ids[0])]
            if kinds[b] == "tie64":
                s[seen] = np.minimum(s[seen], np.float32(1.0))
        elif b % 2 == 0:
            seen = np.union1d(seen, [seen_item]).astype(np.int32)
        scores[b] = s
        seen_lists[int(user_ids[b])] = seen
    for u in range(nu):                                 # users outside the block: lists the call must not read for these rows
        if u not in user_ids:
            seen_lists[u] = np.arange(n, dtype=np.int32)[:: 2]
    targets = _targets(n, T, rng, seen_item)
    for a in [scores, user_ids, targets] + seen_lists:
        a.setflags(write=False)
    return {"I": n, "nb": nb, "K": K, "T": T, "kinds": kinds, "scores": scores, "user_ids": user_ids, "seen_lists": tuple(seen_lists),
            "targets": targets, "name": f"I{n}-nb{nb}-K{K}-T{T}"}


SEL_CASES = tuple([(n, nb, 100, 4) for n in EDGE_I for nb in (1, 3, 4, 5)]
                  + [(n, 5, K, 1) for n in FORM_I for K in K_AXIS]
                  + [(n, 5, 100, T) for n in FORM_I for T in T_AXIS])


def sel_id(c):
    return "I%d-nb%d-K%d-T%d" % c


def sel_rows(case):
    """the (name, scores, seen, K, targets) rows of a case"""
    for b in range(case["nb"]):
        yield (f"{case['name']}-row{b}-{case['kinds'][b]}", case["scores"][b], case["seen_lists"][int(case["user_ids"][b])], case["K"],
               case["targets"])


def csr_of(seen_lists):
    ptr = np.zeros(len(seen_lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(s) for s in seen_lists])
    idx = np.concatenate(list(seen_lists) + [np.zeros(1, dtype=np.int32)]).astype(np.int32)     # (never empty)
    return ptr, idx


@functools.lru_cache(maxsize=None)
def nonfinite_case(n):
    """The patterns of test_topk_rows_nan_scores_same_in_both_kernels, at one catalogue per selection form: per row four quiet
    positive NaNs with distinct payloads, four negative NaNs, two signalling NaNs, a +inf and a -inf; row 1 has a NaN, row 2 the
    -inf, row 3 a negative NaN as targets; in row 4 all but 40 items are seen."""
    rng = np.random.default_rng(_seed(n, 5))
    nb, K = 5, 100
    scores = rng.standard_normal((nb, n), dtype=np.float32)
    b32 = scores.view(U32)
    targets = np.array([3, n - 1, n // 2, 11], dtype=np.int32)
    free = np.setdiff1d(np.arange(n), targets)
    for b in range(nb):
        pos = rng.choice(free, size=12, replace=False)
        b32[b, pos[:4]] = U32(0x7fc00001) + np.arange(4, dtype=U32)
        b32[b, pos[4:8]] = U32(0xffc00000) + np.arange(4, dtype=U32)
        b32[b, pos[8:10]] = U32(0x7f800001) + np.arange(2, dtype=U32)
        scores[b, pos[10]] = np.inf
        scores[b, pos[11]] = -np.inf
    b32[1, 3] = U32(0x7fc00123)
    scores[2, n - 1] = -np.inf
    b32[3, n // 2] = U32(0xffc00001)
    scores[3, 11] = np.inf
    seen_lists = [np.sort(rng.choice(n, size=int(rng.integers(0, 40)), replace=False)).astype(np.int32) for _ in range(nb)]
    seen_lists[4] = np.setdiff1d(np.arange(n), rng.choice(n, size=40, replace=False)).astype(np.int32)
    return {"I": n, "nb": nb, "K": K, "T": 4, "kinds": ("nonfinite",) * nb, "scores": scores, "user_ids": np.arange(nb, dtype=np.int32),
            "seen_lists": tuple(seen_lists), "targets": targets, "name": f"nonfinite-I{n}"}


# ----------------------------------------------------------------------------------- scoring + selection cases (rk_score_topk)
PANEL_D = {2: (20, 32), 4: (50, 64), 8: (100, 128), 16: (130, 256)}      # DC -> (a padded k, the full k)
PANEL_T = {1: (0, 1), 4: (2, 4)}                                          # NTG -> n_targets
INST_NB = 37
INST_I = {15: 2000, 8: 1100}


def inst_params(inst):
    """(NTW, DC, NTG, RB) -> (d, T, I, request): the two dims of a DC and the two target counts of an NTG alternate over the table"""
    ntw, dc, ntg, rb = inst
    j = PANEL_INSTANTIATIONS.index(inst)
    d = PANEL_D[dc][(j + j // 2) % 2]
    T = PANEL_T[ntg][(j // 8 + j // 2) % 2]
    return d, T, INST_I[ntw], PANEL_REQUESTS[(ntw, rb)]


def inst_id(inst):
    return "ntw%d-dc%d-ntg%d-rb%d" % inst


def _tables(rng, nu, n, d, bias):
    utab = rng.standard_normal((nu, d), dtype=np.float32)
    itab = rng.standard_normal((n, d), dtype=np.float32)
    ub = rng.standard_normal(nu, dtype=np.float32) if bias else None
    ib = rng.standard_normal(n, dtype=np.float32) if bias else None
    return utab, itab, ub, ib


def _finish(c):
    """adds the reference scores of the block's rows (computed once, shared, read-only)"""
    uid = c["user_ids"]
    c["ref"] = score_rows(c["utab"][uid], c["itab"], None if c["ub"] is None else c["ub"][uid], c["ib"], c["mean"])
    c["seen_lists"] = tuple(np.asarray(s, dtype=np.int32) for s in c["seen_lists"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def ref_rows(c, nb=None):
    """select_row over the first nb rows of a scoring case -> four stacked arrays"""
    nb = len(c["user_ids"]) if nb is None else nb
    rows = [select_row(c["ref"][b], c["seen_lists"][int(c["user_ids"][b])], c["K"], c["targets"]) for b in range(nb)]
    return tuple(np.stack([r[j] for r in rows]) for j in range(4))


@functools.lru_cache(maxsize=None)
def inst_case(inst):
    d, T, n, request = inst_params(inst)
    rng = np.random.default_rng(_seed(*inst))
    nu, nb, K = INST_NB + 8, INST_NB, 100
    bias = PANEL_INSTANTIATIONS.index(inst) % 2 == 1
    utab, itab, ub, ib = _tables(rng, nu, n, d, bias)
    itab[17] = itab[18] = itab[n - 300]                   # exact ties, the last one in the second panel
    if bias:
        ib[17] = ib[18] = ib[n - 300]
    user_ids = rng.permutation(nu)[:nb].astype(np.int32)
    user_ids[-1] = user_ids[1]
    seen_lists = [np.sort(rng.choice(n, size=int(rng.integers(0, 60)), replace=False)) for _ in range(nu)]
    seen_lists[int(user_ids[3])] = np.sort(rng.choice(n, size=n - 40, replace=False))       # fewer than K unseen
    seen_lists[int(user_ids[5])] = np.union1d(seen_lists[int(user_ids[5])], [17])            # a seen target
    targets = np.asarray([17, 0, n - 1, 17][:T], dtype=np.int32)
    return _finish({"name": inst_id(inst), "d": d, "I": n, "K": K, "T": T, "request": request, "utab": utab, "itab": itab, "ub": ub, "ib": ib,
                    "mean": 0.25 if bias else 0.0, "user_ids": user_ids, "seen_lists": seen_lists, "targets": targets})


# panel edges: one instantiation of RB 1 and one of RB 2 (the narrow form below 1025 items whatever was asked: score_topk.hip:753)
EDGE_REQUESTS = {"rows16": {"path": "panel", "panel_rows": 16}, "rows32": {"path": "panel", "panel_rows": 32}}
PANEL_EDGE_I = (1, 15, 16, 17, 1024, 1025, 1920, 1921, 3840, 3841)
PANEL_EDGE_NB = (1, 15, 16, 17, 31, 32, 33)
PANEL_EDGE_K = (1, 255, 256)
SEEN_IN_PANEL = (0, 31, 32, 33, 64, 65)
EDGE_USERS = 40
TIE_PAIRS = ((1919, 1920, 500.0), (1023, 1024, 400.0))


@functools.lru_cache(maxsize=None)
def edge_case(n, K=100):
    """d = 64, one target, biases.  Users 0-5 have exactly 0 / 31 / 32 / 33 / 64 / 65 seen ids inside the first panel (as many as
    the catalogue has), user 6 all of its seen ids in the second panel, user 7 item I - 1 alone, user 8 the whole first panel (1920
    items; it covers the narrow one), user 9 everything; the rest random lists.  Items 1919 / 1920 and 1023 / 1024 score the same
    for every user and lead every list (item biases of +500 and +400): ties across the boundary of a 1920- and of a 1024-item panel."""
    rng = np.random.default_rng(_seed(n, K, 77))
    nu, d = EDGE_USERS, 64
    utab, itab, ub, ib = _tables(rng, nu, n, d, True)
    for lo, hi, lift in TIE_PAIRS:
        if hi < n:
            itab[hi] = itab[lo]
            ib[lo] = ib[hi] = np.float32(lift)
    pi = min(n, 1920)
    seen_lists = [np.sort(rng.choice(n, size=int(rng.integers(0, min(n, 60) + 1)), replace=False)) for _ in range(nu)]
    for u, cnt in enumerate(SEEN_IN_PANEL):
        seen_lists[u] = np.unique((np.arange(cnt) * 29 + 5) % min(n, 1024))
        assert len(seen_lists[u]) == min(cnt, min(n, 1024)) or n < 65
    seen_lists[6] = np.arange(1920, min(n, 3840))[::7] if n > 1920 else np.arange(1024, n)[::3]
    seen_lists[7] = np.array([n - 1])
    seen_lists[8] = np.arange(pi)
    seen_lists[9] = np.arange(n)
    user_ids = np.r_[np.arange(10), rng.permutation(np.arange(10, nu))[:23]].astype(np.int32)          # 33 rows
    user_ids[-1] = 4
    targets = np.asarray([min(1920, n - 1)], dtype=np.int32)
    return _finish({"name": f"edge-I{n}-K{K}", "d": d, "I": n, "K": K, "T": 1, "utab": utab, "itab": itab, "ub": ub, "ib": ib, "mean": 0.125,
                    "user_ids": user_ids, "seen_lists": seen_lists, "targets": targets})


@functools.lru_cache(maxsize=None)
def bias_case():
    """ub = 1e4, ib = -1e4 + small, mean = 1e-3: ((dot + ub) + ib) + mean loses the low bits of dot and of `small` in the first
    sum and keeps what is left through the cancellation; any other association keeps other bits."""
    rng = np.random.default_rng(4242)
    nu, n, d = 40, 1300, 64
    utab, itab, _, _ = _tables(rng, nu, n, d, False)
    ub = np.full(nu, 1e4, dtype=np.float32)
    ib = (np.float32(-1e4) + rng.uniform(0.0, 0.5, n).astype(np.float32)).astype(np.float32)
    user_ids = rng.permutation(nu)[:INST_NB].astype(np.int32)
    seen_lists = [np.sort(rng.choice(n, size=int(rng.integers(0, 60)), replace=False)) for _ in range(nu)]
    return _finish({"name": "bias-order", "d": d, "I": n, "K": 100, "T": 1, "utab": utab, "itab": itab, "ub": ub, "ib": ib, "mean": 1e-3,
                    "user_ids": user_ids, "seen_lists": seen_lists, "targets": np.asarray([5], dtype=np.int32)})


NONFINITE_ITEMS = {"nan": 700, "pos_inf": 1100, "neg_inf": 1500}
NEG_INF_IN_FRONT = (300, 1499)       # two more -inf items in front of the -inf target: another tile, and its own 16-item tile


@functools.lru_cache(maxsize=None)
def nonfinite_tables_case(with_nan=True):
    """Training gone wrong: item 1100's row holds 3e38 and item 1500's -3e38 (and so do items 300 and 1499, two -inf scores in FRONT of the -inf target, in another 16-item tile and in its
    own) in every k against user rows that are positive in
    every k, so their fmaf chains overflow to +inf and -inf from FINITE tables without ever meeting the opposite infinity; with_nan:
    item 700's row is NaN as well (the quiet positive NaN 0x7fc00000 in every k).  No NaN is PRODUCED anywhere: what a NaN that the
    hardware makes looks like is not this test's subject.  Targets: the three items and an ordinary one.  User 3 has seen all but
    40 items -- the three special ones are among the unseen -- so its list is shorter than K; user 5 has seen item 700, user 7
    item 1500, user 9 item 300."""
    rng = np.random.default_rng(977)
    nu, n, d, K = 45, 2000, 64, 100
    utab, itab, ub, ib = _tables(rng, nu, n, d, True)
    utab = (np.abs(utab) + np.float32(0.5)).astype(np.float32)
    if with_nan:
        itab[NONFINITE_ITEMS["nan"]] = np.float32(np.nan)
        assert bits(itab[NONFINITE_ITEMS["nan"]])[0] == 0x7fc00000
    itab[NONFINITE_ITEMS["pos_inf"]] = np.float32(3e38)
    itab[NONFINITE_ITEMS["neg_inf"]] = np.float32(-3e38)
    itab[list(NEG_INF_IN_FRONT)] = np.float32(-3e38)
    user_ids = rng.permutation(nu)[:INST_NB].astype(np.int32)
    seen_lists = [np.sort(rng.choice(n, size=int(rng.integers(0, 60)), replace=False)) for _ in range(nu)]
    special = np.asarray(sorted(list(NONFINITE_ITEMS.values()) + list(NEG_INF_IN_FRONT)))
    for u in range(nu):
        seen_lists[u] = np.setdiff1d(seen_lists[u], special)
    keep = np.union1d(rng.choice(n, size=37, replace=False), special)
    seen_lists[int(user_ids[3])] = np.setdiff1d(np.arange(n), keep)
    seen_lists[int(user_ids[5])] = np.union1d(seen_lists[int(user_ids[5])], [NONFINITE_ITEMS["nan"]])
    seen_lists[int(user_ids[7])] = np.union1d(seen_lists[int(user_ids[7])], [NONFINITE_ITEMS["neg_inf"]])
    seen_lists[int(user_ids[9])] = np.union1d(seen_lists[int(user_ids[9])], [NEG_INF_IN_FRONT[0]])
    targets = np.asarray([NONFINITE_ITEMS["nan"], NONFINITE_ITEMS["pos_inf"], NONFINITE_ITEMS["neg_inf"], 9], dtype=np.int32)
    return _finish({"name": "nonfinite-tables" if with_nan else "overflowing-tables", "d": d, "I": n, "K": K, "T": 4, "utab": utab, "itab": itab,
                    "ub": ub, "ib": ib, "mean": 0.25, "user_ids": user_ids, "seen_lists": seen_lists, "targets": targets})
