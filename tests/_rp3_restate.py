"""Numpy restatement of the RP3beta definition (include/recad_hip.h): the 40-bit fixed-point steps, the factors, the dots as
uint64 sums, the weight formed in float64 and rounded once to float32, candidates ordered by the 64-bit key, scores summed in
fp32 in ascending item order.  The kernels of csrc/rp3beta.hip are compared with it bit for bit.  Beside it: the float64
textbook RP3beta from dense products, the float64 evaluation of the kept tables and the counted score budget."""
import numpy as np

from tests import _knn_restate as K

SCALE = 2.0 ** 40
U24 = 2.0 ** -24
# score budget: w carries 1 fp32 rounding against its float64 value, the term 1 more, the m - 1 adds of m terms one each: m + 1
# roundings, |error| <= gamma_(m+1) * sum, gamma_n = n u / (1 - n u) <= (n + 1) u while n (n + 1) u <= 1, that is m <= 4094
SCORE_C = 2


def dense(ptr, idx, val, n_items):
    return K.dense(ptr, idx, val, n_items)


def _power(x, e):
    """x ** e with the two exact cases of the definition."""
    x = np.asarray(x, dtype=np.float64)
    if e == 1:
        return x.copy()
    if e == 0:
        return np.ones_like(x)
    return np.power(x, np.float64(e))


def steps(ptr, idx, val, alpha):
    """(P int64 [nnz], r int64 [U]): P = max(1, rint(2^40 * (q / r_u) ** alpha))."""
    q = np.asarray(val, dtype=np.float32).astype(np.int64)
    U = len(ptr) - 1
    row = np.repeat(np.arange(U), np.diff(ptr))
    r = np.zeros(U, dtype=np.int64)
    np.add.at(r, row, q)
    p = _power(q.astype(np.float64) / r[row].astype(np.float64), alpha)
    return np.maximum(1, np.rint(SCALE * p).astype(np.int64)), r


def factors(n, alpha, beta):
    """(fa, fb) float64 [I] from the rater counts: n ** -alpha and n ** -beta, 0 for an unrated item."""
    n = np.asarray(n, dtype=np.int64)
    safe = np.maximum(n, 1).astype(np.float64)

    def one(e):
        f = 1.0 / safe if e == 1 else np.ones_like(safe) if e == 0 else np.power(safe, -np.float64(e))
        return np.where(n > 0, f, 0.0)

    return one(alpha), one(beta)


def dots(ptr, idx, P, n_items, first=None):
    """S uint64 [I, I]: S_ij = sum over the raters u of i of P_uj (diagonal included; the neighbour step drops it).  `first`
    ([nnz] integers) replaces the binarised first step, for the variant tests."""
    U = len(ptr) - 1
    row = np.repeat(np.arange(U), np.diff(ptr))
    B, Pd = np.zeros((U, n_items), dtype=np.uint64), np.zeros((U, n_items), dtype=np.uint64)
    B[row, idx] = 1 if first is None else np.asarray(first, dtype=np.uint64)
    Pd[row, idx] = np.asarray(P, dtype=np.int64).astype(np.uint64)
    S = np.zeros((n_items, n_items), dtype=np.uint64)
    for u in range(U):                                                 # integer outer products: exact, no BLAS
        c = idx[ptr[u]:ptr[u + 1]]
        S[np.ix_(c, c)] += B[u, c][:, None] * Pd[u, c][None, :]
    return S


def weights(S, fa, fb):
    """float32 [I, I]: (float)((((double) S * fa_i) * fb_j) * 2^-40)."""
    return (((S.astype(np.float64) * fa[:, None]) * fb[None, :]) * (1.0 / SCALE)).astype(np.float32)


def weights64(S, fa, fb):
    """The same product before its rounding to float32."""
    return ((S.astype(np.float64) * fa[:, None]) * fb[None, :]) * (1.0 / SCALE)


def neighbours_from(S, W, k):
    """(nbr_id int32 [k, I], nbr_w float32 [k, I]), slot-major, from the dots and the fp32 weights: candidates j != i with
    S_ij > 0 by the key (bits of w) << 32 | (0xFFFFFFFF - j) descending; unused slots hold -1 and +0.0."""
    I = S.shape[0]
    k_eff = min(k, I - 1)
    nbr_id, nbr_w = np.full((k, I), -1, dtype=np.int32), np.zeros((k, I), dtype=np.float32)
    bits = np.ascontiguousarray(W, dtype=np.float32).view(np.uint32).astype(np.uint64)
    for i in range(I):
        cand = np.nonzero(S[i] > 0)[0]
        cand = cand[cand != i]
        key = (bits[i, cand] << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - cand.astype(np.uint64))
        cand = cand[np.argsort(key)[::-1]][:k_eff]                     # the keys are distinct
        nbr_id[: len(cand), i], nbr_w[: len(cand), i] = cand, W[i, cand]
    return nbr_id, nbr_w


def fit_parts(ptr, idx, val, n_items, alpha, beta):
    """(P, r, fa, fb) of the definition."""
    P, r = steps(ptr, idx, val, alpha)
    fa, fb = factors(np.bincount(idx, minlength=n_items), alpha, beta)
    return P, r, fa, fb


def neighbours(ptr, idx, val, n_items, k, alpha, beta, P=None, fa=None, fb=None):
    """The tables of the definition; P / fa / fb given: the tables of those inputs (what rk_rp3_neighbors computes from them)."""
    P0, _, fa0, fb0 = fit_parts(ptr, idx, val, n_items, alpha, beta)
    P, fa, fb = (P0 if P is None else P), (fa0 if fa is None else fa), (fb0 if fb is None else fb)
    S = dots(ptr, idx, P, n_items)
    return neighbours_from(S, weights(S, fa, fb), k)


def textbook(ptr, idx, val, n_items, alpha, beta):
    """W float64 [I, I] of RP3beta from dense float64 products: W_ij = sum_u (1 / n_i)^alpha (q_uj / r_u)^alpha / n_j^beta over
    the raters u of i (the first step binarised); rows and columns of unrated items are 0."""
    A = dense(ptr, idx, val, n_items).astype(np.float64)
    B = (A > 0).astype(np.float64)
    r = np.maximum(A.sum(axis=1), 1.0)
    n = B.sum(axis=0)
    Pui = np.where(A > 0, np.power(A / r[:, None], alpha), 0.0)
    with np.errstate(divide="ignore"):
        fa = np.where(n > 0, np.power(np.maximum(n, 1.0), -alpha), 0.0)
        fb = np.where(n > 0, np.power(np.maximum(n, 1.0), -beta), 0.0)
    return (B.T @ Pui) * fa[:, None] * fb[None, :]


def _walk(A, nbr_id, nbr_w, users, descending=False):
    """(scores float32 [n, I], m int64 [n, I] the number of terms of every score).  For every user the items in ascending order
    (descending: the variant the definition rules out), and for each the kept list scattered into the row:
    row[id] = fl(row[id] + fl(w * (float) q))."""
    users = np.asarray(users, dtype=np.int64)
    I = A.shape[1]
    out, m = np.zeros((len(users), I), dtype=np.float32), np.zeros((len(users), I), dtype=np.int64)
    for b, u in enumerate(users):
        items = np.nonzero(A[u])[0]
        for i in (items[::-1] if descending else items):
            ids, w = nbr_id[:, i], nbr_w[:, i]
            ok = ids >= 0
            term = (w[ok] * np.float32(A[u, i])).astype(np.float32)    # one rounding, then the add: never fused
            out[b, ids[ok]] = (out[b, ids[ok]] + term).astype(np.float32)   # the ids of one list are distinct
            m[b, ids[ok]] += 1
    return out, m


def scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, descending=False):
    """float32 [len(users), I]."""
    return _walk(dense(ptr, idx, val, n_items), nbr_id, nbr_w, users, descending)[0]


def term_counts(ptr, idx, val, n_items, nbr_id, nbr_w, users):
    """m int64 [len(users), I]: how many terms each score sums."""
    return _walk(dense(ptr, idx, val, n_items), nbr_id, nbr_w, users)[1]


def pair_scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, items):
    """float32 [n]; a pair with a user or item id out of range scores 0.0."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    A = dense(ptr, idx, val, n_items)
    ok = (users >= 0) & (users < A.shape[0]) & (items >= 0) & (items < n_items)
    out = np.zeros(len(users), dtype=np.float32)
    if ok.any():
        uniq, inv = np.unique(users[ok], return_inverse=True)
        rows = _walk(A, nbr_id, nbr_w, uniq)[0]
        out[ok] = rows[inv, items[ok]]
    return out


def scores_exact(ptr, idx, val, n_items, nbr_id, users, alpha, beta):
    """float64 [len(users), I]: the same kept ids with w = ((S fa_i) fb_j) 2^-40 in float64, before its rounding to fp32: the
    bound's sum of terms."""
    A = dense(ptr, idx, val, n_items)
    P, _, fa, fb = fit_parts(ptr, idx, val, n_items, alpha, beta)
    W = weights64(dots(ptr, idx, P, n_items), fa, fb)
    users = np.asarray(users, dtype=np.int64)
    out = np.zeros((len(users), n_items))
    for b, u in enumerate(users):
        for i in np.nonzero(A[u])[0]:
            ids = nbr_id[:, i]
            ids = ids[ids >= 0]
            out[b, ids] += W[i, ids] * float(A[u, i])
    return out


def score_budget(m, exact):
    """(m + SCORE_C) * 2^-24 * the sum of the terms."""
    return (m + SCORE_C) * U24 * exact


def topk_unseen(row, seen, K):
    """Ids of the K best unseen items of one score row: score descending, ties to the lower id."""
    s = np.asarray(row, dtype=np.float64).copy()
    s[np.asarray(seen, dtype=np.int64)] = -np.inf
    order = np.lexsort((np.arange(len(s)), -s))
    return order[: min(K, len(s) - len(seen))]


def hit_ratio(ptr, idx, val, n_items, k, alpha, beta, target, K, real_users=None):
    """(HR@K of `target` over the users of [0, real_users) who have not rated it, how many such users): the restated model fitted
    on the whole CSR."""
    nbr_id, nbr_w = neighbours(ptr, idx, val, n_items, k, alpha, beta)
    U = len(ptr) - 1 if real_users is None else real_users
    users = [u for u in range(U) if target not in idx[ptr[u]:ptr[u + 1]]]
    S = scores(ptr, idx, val, n_items, nbr_id, nbr_w, users)
    hits = sum(target in topk_unseen(S[r], idx[ptr[u]:ptr[u + 1]], K) for r, u in enumerate(users))
    return hits / max(len(users), 1), len(users)
