"""Numpy restatement of the UserKNN definition (include/recad_hip.h): an int64 dense A @ A.T, float32 operations in the stated
order (those of tests/_knn_restate.py), candidates ordered by (w descending, id ascending), scores summed in slot order over the
kept neighbours who rated the item, and with `normalize` the weighted average by one fp32 division.  The kernels of
csrc/userknn.hip, and rk_itemknn_neighbors on the transposed roles, are compared with it bit for bit."""
import numpy as np

from tests import _knn_restate as K
from tests._itemknn_restate import topk_unseen


def dense(ptr, idx, val, n_items):
    return K.dense(ptr, idx, val, n_items)


def similarities(A):
    """(D int64 [U, U], W float32 [U, U]): w_uv = ((float) d_uv * r_u) * r_v."""
    D = A @ A.T
    r = K.rnorm(A)
    return D, (D.astype(np.float32) * r[:, None]) * r[None, :]


def neighbours(ptr, idx, val, n_items, k):
    """(nbr_id int32 [k, U], nbr_w float32 [k, U]), slot-major; unused slots hold -1 and +0.0."""
    D, W = similarities(dense(ptr, idx, val, n_items))
    U = D.shape[0]
    k_eff = min(k, U - 1)
    nbr_id, nbr_w = np.full((k, U), -1, dtype=np.int32), np.zeros((k, U), dtype=np.float32)
    for u in range(U):
        cand = np.nonzero(D[u] > 0)[0]
        cand = cand[cand != u]
        cand = cand[np.lexsort((cand, -W[u, cand].astype(np.float64)))][:k_eff]      # w descending, then id ascending
        nbr_id[: len(cand), u], nbr_w[: len(cand), u] = cand, W[u, cand]
    return nbr_id, nbr_w


def _finish(s, den, normalize):
    if not normalize:
        return s
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (s / den).astype(np.float32), np.float32(0)).astype(np.float32)


def _rows(A, nbr_id, nbr_w, users, normalize, items=None):
    """s <- s + fl(w_t * (float) q_vj), den <- den + w_t, t ascending, over the slots whose neighbour v rated j: for the given
    users (in [0, U)) and every item, or, with `items`, for the pairs (users[p], items[p])."""
    U, I = A.shape
    users = np.asarray(users, dtype=np.int64)
    n = len(users)
    s = np.zeros((n, I) if items is None else n, dtype=np.float32)
    den = np.zeros_like(s)
    Af = A.astype(np.float32)
    for t in range(nbr_id.shape[0]):
        v, w = nbr_id[t, users].astype(np.int64), nbr_w[t, users]
        ok = (v >= 0) & (v < U)                                        # -1 and a foreign id are skipped
        vv = np.where(ok, v, 0)
        if items is None:
            q = Af[vv]                                                 # [n, I]
            hit = ok[:, None] & (q != 0)
            wt = np.broadcast_to(w[:, None], q.shape)
        else:
            q = Af[vv, np.asarray(items, dtype=np.int64)]
            hit = ok & (q != 0)
            wt = w
        term = (wt * q).astype(np.float32)                             # one rounding, then the add: never fused
        s = np.where(hit, (s + term).astype(np.float32), s)
        den = np.where(hit, (den + wt).astype(np.float32), den)
    return _finish(s, den, normalize)


def scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, normalize=False):
    """float32 [len(users), I]; a user id outside [0, U) scores +0.0 everywhere."""
    A = dense(ptr, idx, val, n_items)
    users = np.asarray(users, dtype=np.int64)
    ok = (users >= 0) & (users < A.shape[0])
    out = np.zeros((len(users), n_items), dtype=np.float32)
    if ok.any():
        out[ok] = _rows(A, nbr_id, nbr_w, users[ok], normalize)
    return out


def pair_scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, items, normalize=False):
    """float32 [n]; a pair with a user or item id out of range scores 0.0."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    A = dense(ptr, idx, val, n_items)
    ok = (users >= 0) & (users < A.shape[0]) & (items >= 0) & (items < n_items)
    out = np.zeros(len(users), dtype=np.float32)
    if ok.any():
        out[ok] = _rows(A, nbr_id, nbr_w, users[ok], normalize, items[ok])
    return out


def scores_exact(ptr, idx, val, n_items, nbr_id, users, normalize=False):
    """float64 scores of the SAME neighbour lists with w = d_uv / sqrt(n_u n_v) in float64: un-normalised the bound's
    sum_t w_t q_t, normalised the float64 quotient (0 where no kept neighbour rated the item)."""
    A = dense(ptr, idx, val, n_items)
    D = (A @ A.T).astype(np.float64)
    n = np.maximum(np.diag(D), 1.0)
    W = D / np.sqrt(np.outer(n, n))
    users = np.asarray(users, dtype=np.int64)
    Af = A.astype(np.float64)
    s, den = np.zeros((len(users), n_items)), np.zeros((len(users), n_items))
    for t in range(nbr_id.shape[0]):
        v = nbr_id[t, users].astype(np.int64)
        ok = v >= 0
        vv = np.where(ok, v, 0)
        w = np.where(ok, W[users, vv], 0.0)[:, None]
        q = Af[vv]
        hit = ok[:, None] & (q != 0)
        s += np.where(hit, w * q, 0.0)
        den += np.where(hit, w, 0.0)
    if not normalize:
        return s
    return np.where(den > 0, s / np.where(den > 0, den, 1.0), 0.0)


def hit_ratio(ptr, idx, val, n_items, k, target, K, real_users=None, normalize=False):
    """(HR@K of `target` over the users of [0, real_users) who have not rated it, how many such users): the restated model fitted
    on the whole CSR."""
    nbr_id, nbr_w = neighbours(ptr, idx, val, n_items, k)
    U = len(ptr) - 1 if real_users is None else real_users
    users = [u for u in range(U) if target not in idx[ptr[u]:ptr[u + 1]]]
    S = scores(ptr, idx, val, n_items, nbr_id, nbr_w, users, normalize)
    hits = sum(target in topk_unseen(S[r], idx[ptr[u]:ptr[u + 1]], K) for r, u in enumerate(users))
    return hits / max(len(users), 1), len(users)
