"""Numpy restatement of the ItemKNN definition (include/recad_hip.h): an int64 dense A.T @ A, float32 operations in the stated
order, candidates ordered by (w descending, id ascending), scores summed in slot order.  The kernels of csrc/itemknn.hip are
compared with it bit for bit."""
import numpy as np

from tests import _knn_restate as K


def dense(ptr, idx, val, n_items):
    return K.dense(ptr, idx, val, n_items)


def item_rnorm(A):
    """r_i of every column: rk_knn_norms applied to the transpose."""
    return K.rnorm(np.ascontiguousarray(A.T))


def similarities(A):
    """(D int64 [I, I], W float32 [I, I]): w_ij = ((float) d_ij * r_i) * r_j."""
    D = A.T @ A
    r = item_rnorm(A)
    return D, (D.astype(np.float32) * r[:, None]) * r[None, :]


def neighbours(ptr, idx, val, n_items, k):
    """(nbr_id int32 [k, I], nbr_w float32 [k, I]), slot-major; unused slots hold -1 and +0.0."""
    D, W = similarities(dense(ptr, idx, val, n_items))
    I, k_eff = n_items, min(k, n_items - 1)
    nbr_id, nbr_w = np.full((k, I), -1, dtype=np.int32), np.zeros((k, I), dtype=np.float32)
    for i in range(I):
        cand = np.nonzero(D[i] > 0)[0]
        cand = cand[cand != i]
        cand = cand[np.lexsort((cand, -W[i, cand].astype(np.float64)))][:k_eff]      # w descending, then id ascending
        nbr_id[: len(cand), i], nbr_w[: len(cand), i] = cand, W[i, cand]
    return nbr_id, nbr_w


def _rows(A, nbr_id, nbr_w, users, items=None):
    """s_{t+1} = s_t + fl(w_t * (float) q), t ascending, for the given users (rows of the result) and every item, or, with
    `items`, for the pairs (users[p], items[p])."""
    users = np.asarray(users, dtype=np.int64)
    Q = A[users].astype(np.float32)                                   # [n, I]
    n, I = Q.shape
    cols = np.arange(I) if items is None else np.asarray(items, dtype=np.int64)
    s = np.zeros((n, I) if items is None else n, dtype=np.float32)
    for t in range(nbr_id.shape[0]):
        ids, w = nbr_id[t, cols], nbr_w[t, cols]
        q = Q[:, np.maximum(ids, 0)] if items is None else Q[np.arange(n), np.maximum(ids, 0)]
        term = (w * q).astype(np.float32)                             # one rounding, then the add: never fused
        s = np.where(ids >= 0, (s + term).astype(np.float32), s)
    return s


def scores(ptr, idx, val, n_items, nbr_id, nbr_w, users):
    """float32 [len(users), I]."""
    return _rows(dense(ptr, idx, val, n_items), nbr_id, nbr_w, users)


def pair_scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, items):
    """float32 [n]; a pair with a user or item id out of range scores 0.0."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    A = dense(ptr, idx, val, n_items)
    ok = (users >= 0) & (users < A.shape[0]) & (items >= 0) & (items < n_items)
    out = np.zeros(len(users), dtype=np.float32)
    if ok.any():
        out[ok] = _rows(A, nbr_id, nbr_w, users[ok], items[ok])
    return out


def scores_exact(ptr, idx, val, n_items, nbr_id, users):
    """(float64 scores of the SAME neighbour lists, with w = d_ij / sqrt(n_i n_j) in float64; the bound's sum_t w_t q_t)."""
    A = dense(ptr, idx, val, n_items)
    D = (A.T @ A).astype(np.float64)
    n = np.maximum(np.diag(D), 1.0)
    W = D / np.sqrt(np.outer(n, n))
    Q = A[np.asarray(users, dtype=np.int64)].astype(np.float64)
    s = np.zeros((Q.shape[0], n_items))
    for t in range(nbr_id.shape[0]):
        ids = nbr_id[t]
        s += np.where(ids >= 0, W[np.arange(n_items), np.maximum(ids, 0)] * Q[:, np.maximum(ids, 0)], 0.0)
    return s


def topk_unseen(row, seen, K):
    """Ids of the K best unseen items of one score row: score descending, ties to the lower id."""
    s = np.asarray(row, dtype=np.float64).copy()
    s[np.asarray(seen, dtype=np.int64)] = -np.inf
    order = np.lexsort((np.arange(len(s)), -s))
    return order[: min(K, len(s) - len(seen))]


def hit_ratio(ptr, idx, val, n_items, k, target, K, real_users=None):
    """(HR@K of `target` over the users of [0, real_users) who have not rated it, how many such users): the restated model fitted
    on the whole CSR."""
    nbr_id, nbr_w = neighbours(ptr, idx, val, n_items, k)
    U = len(ptr) - 1 if real_users is None else real_users
    users = [u for u in range(U) if target not in idx[ptr[u]:ptr[u + 1]]]
    S = scores(ptr, idx, val, n_items, nbr_id, nbr_w, users)
    hits = sum(target in topk_unseen(S[r], idx[ptr[u]:ptr[u + 1]], K) for r, u in enumerate(users))
    return hits / max(len(users), 1), len(users)
