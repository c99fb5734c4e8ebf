"""Numpy restatement of the KnnSelectUsers definition (include/recad_hip.h): an int64 dense A @ A.T, float32 operations in the
stated order, a sequential float64 sum.  The kernels of csrc/knn.hip are compared with it bit for bit."""
import numpy as np

BAD_VALUE, BAD_COLUMN, BAD_NORM = 1, 2, 3


def first_violation(ptr, idx, val, n_items):
    """(rule, row) of the lowest offending row (the lowest rule inside it), or None."""
    for u in range(len(ptr) - 1):
        c, x = np.asarray(idx[ptr[u]:ptr[u + 1]], dtype=np.int64), np.asarray(val[ptr[u]:ptr[u + 1]], dtype=np.float32)
        if not np.all((x >= 1) & (x <= 127) & (x == np.floor(x))):      # false for NaN
            return BAD_VALUE, u
        if np.any(c < 0) or np.any(c >= n_items) or np.any(np.diff(c) <= 0):
            return BAD_COLUMN, u
        if int((x.astype(np.int64) ** 2).sum()) >= 2 ** 31:
            return BAD_NORM, u
    return None


def dense(ptr, idx, val, n_items):
    A = np.zeros((len(ptr) - 1, n_items), dtype=np.int64)
    A[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = np.asarray(val, dtype=np.float32).astype(np.int64)
    return A


def large_dot_odd():
    """Two rows over 1100 items, all 127 but for one 2 in row 1: d_01 = 1099 * 127^2 + 254 is odd and above 2^24."""
    val = np.full(2200, 127.0, dtype=np.float32)
    val[2199] = 2.0
    return np.array([0, 1100, 2200]), np.r_[np.arange(1100), np.arange(1100)].astype(np.int32), val, 1100


def rnorm(A):
    n = (A * A).sum(axis=1)
    return np.where(n > 0, (1.0 / np.sqrt(np.maximum(n, 1).astype(np.float64))).astype(np.float32), np.float32(0))


def mean_of(top, k_eff):
    """(float)(s / k_eff), s the float64 sum of top[0..k_eff) taken one after the other in the order given."""
    s = 0.0
    for x in top[:k_eff]:
        s = s + float(x)
    return np.float32(s / k_eff) if k_eff else np.float32(0)


def degsim(ptr, idx, val, n_items, k):
    """(topw float32 [U, k], degsim float32 [U])."""
    A = dense(ptr, idx, val, n_items)
    U, r = A.shape[0], rnorm(A)
    W = ((A @ A.T).astype(np.float32) * r[:, None]) * r[None, :]
    k_eff = min(k, U - 1)
    topw, out = np.zeros((U, k), dtype=np.float32), np.zeros(U, dtype=np.float32)
    for u in range(U):
        topw[u, :k_eff] = -np.sort(-np.delete(W[u], u), kind="stable")[:k_eff]
        out[u] = mean_of(topw[u], k_eff)
    return topw, out


def select(scores, m, how="low"):
    """The ids of the m smallest ("low") or largest ("high") scores, ties to the lower id; -0.0 equals 0.0."""
    s = np.asarray(scores, dtype=np.float32) + np.float32(0)          # -0.0 + 0.0 = +0.0
    if not np.all(np.isfinite(s)) or not 0 <= m <= len(s):
        raise ValueError("a non-finite score, or m outside 0..n")
    return np.lexsort((np.arange(len(s)), s if how == "low" else -s))[:m].tolist()
