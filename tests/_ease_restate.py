"""Numpy restatement of the EASE definition (include/recad_hip.h) and of the algorithm rk_ease_invert runs (csrc/ease.hip).

The definition: gram() is the int64 X^T X, matrix() the fp32 A with lambda added to the diagonal by one fp32 add, inverse64() the
float64 inverse P* of that fp32 matrix and its condition number, weights() B by the stated double division, scores() /
pair_scores() the fp32 chain over a user's entries in column order.  Gram, weights and scores are compared bit for bit with the
kernels; the inverse is compared within a budget.

The walk: invert_walk() is a plain fp32 numpy walk of the blocked Gauss-Jordan sweep of rk_ease_invert for one block width: per
block K, D = inv(A_KK) by the unblocked sweep of the pivot kernel (gj_unblocked), A_Kj <- D A_Kj, A_ij <- A_ij - A_iK (D A_Kj),
A_iK <- -A_iK D for i, j outside K.  It rounds where numpy's fp32 products round, not where the MFMA chain does: block order
and contraction change which roundings happen, not how many.

Budgets.  e_hard = I * 2^-24 * kappa * max|P*| is the forward bound of a backward-stable SPD inverse with constant 1.  The
device is held per input to e_P = min(e_hard, 4 * (the walk's error on that input) + 2^-23 * max|P*|).
Measured on the inputs of SIZES x CASES (tests/test_ease_host.py prints them), the worst over U in {1, 5, 70, 300} and lambda in
{0.5, 10, 500} per (block, I), as err / max|P*| and as a fraction of e_hard:

  block   I   err / max|P*|   err / e_hard   kappa <=  |  block   I   err / max|P*|   err / e_hard   kappa <=
     32   1        5.8e-08         0.9688          1  |     64   1        5.8e-08         0.9688          1
     32   2        7.3e-08         0.6098          4  |     64   2        7.3e-08         0.6098          4
     32   3        1.5e-07         0.2651        498  |     64   3        1.5e-07         0.2651        498
     32  31        3.9e-07         0.1430       1197  |     64  63        5.3e-07         0.0697       1496
     32  32        5.0e-07         0.1360       1224  |     64  64        5.8e-07         0.1126       1464
     32  33        4.1e-07         0.1390       1258  |     64  65        1.4e-06         0.1078       1550
     32  63        8.1e-07         0.0587       1496  |     64 127        4.2e-06         0.0839       1833
     32  64        2.6e-06         0.0744       1464  |     64 128        3.6e-06         0.0705       1857
     32  65        1.7e-06         0.0779       1550  |     64 129        4.7e-06         0.0786       1861
     32 101        3.0e-06         0.0632       1770  |     64 197        6.8e-06         0.0601       2072
   auto 200        4.4e-06         0.0413       2052  |   auto 257        6.6e-06         0.0432       2308

(At I = 1 the inverse is one correctly rounded division, half an ulp: all of the bound's 2^-24.)

From e_P (a bound on every |P_ij - P*_ij|, u = 2^-24):
  B.  B_ij = -fl(P_ij / P_jj), the quotient formed in double (its own rounding, 2^-53, is neglected) and rounded once to fp32.
      P_ij / P_jj - P*_ij / P*_jj = ((P_ij - P*_ij) + B*_ij (P_jj - P*_jj)) / P_jj with B*_ij = -P*_ij / P*_jj and
      P_jj >= P*_jj - e_P > 0, so t_ij = e_P (1 + |B*_ij|) / (P*_jj - e_P) bounds the quotient's error and
      e_B[i, j] = t_ij + u (|B*_ij| + t_ij) the weight's (b_budget).
  score.  s = the chain of n terms fl(q_e B[i_e, j]): one rounding per term and one per add, so by the standard bound of a
      recursive sum |s - sum_e q_e B[i_e, j]| <= g_n sum_e q_e |B[i_e, j]|, g_n = n u / (1 - n u), and with |B| <= |B*| + e_B
      e_S[u, j] = sum_e q_e e_B[i_e, j] + g_n sum_e q_e (|B*[i_e, j]| + e_B[i_e, j]) (score_budget)."""
import functools

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
BLOCKS = (32, 64)


# ------------------------------------------------------------------------------------------------------------ the definition
def dense(ptr, idx, val, n_items):
    """int64 [U, I] of a rating CSR."""
    U = len(ptr) - 1
    A = np.zeros((U, n_items), dtype=np.int64)
    A[np.repeat(np.arange(U), np.diff(ptr)), idx] = np.asarray(val).astype(np.int64)
    return A


def gram(X):
    """d_ij in int64."""
    X = np.asarray(X, dtype=np.int64)
    return X.T @ X


def matrix(D, lam):
    """The fp32 A: (float) d_ij, and (float) d_ii + lambda by one fp32 add."""
    assert np.all(np.diag(D) < 2 ** 24)
    A = D.astype(F32)
    i = np.arange(len(A))
    A[i, i] = (A[i, i] + F32(lam)).astype(F32)
    return A


def inverse64(A):
    """(P* = inv of the float64 copy of A, kappa = the ratio of its extreme eigenvalues)."""
    A64 = np.asarray(A, dtype=np.float64)
    w = np.linalg.eigvalsh(A64)
    return np.linalg.inv(A64), float(w[-1] / w[0])


def weights(P):
    """B (fp32) from P (fp32 or float64): -(float)((double) P_ij / (double) P_jj), +0.0 on the diagonal."""
    P = np.asarray(P, dtype=np.float64)
    B = -(P / np.diag(P)[None, :]).astype(F32)
    B[np.arange(len(B)), np.arange(len(B))] = F32(0)
    return B


def _chain(Q, B, cols=None):
    """s_{e+1} = s_e + fl(q * B[i, j]) over the items i of each row of Q (float32 [n, I]) in ascending order, for every j or,
    with cols, for column cols[r] of row r."""
    n, I = Q.shape
    s = np.zeros((n, I) if cols is None else n, dtype=F32)
    for i in range(I):
        q = Q[:, i]
        if not q.any():
            continue
        if cols is None:
            term = (q[:, None] * B[i][None, :]).astype(F32)            # one rounding, then the add: never fused
            s = np.where(q[:, None] > 0, (s + term).astype(F32), s)
        else:
            term = (q * B[i, cols]).astype(F32)
            s = np.where(q > 0, (s + term).astype(F32), s)
    return s


def scores(X, B, users):
    """float32 [len(users), I]; X the dense int64 rating matrix."""
    return _chain(X[np.asarray(users, dtype=np.int64)].astype(F32), np.asarray(B, dtype=F32))


def pair_scores(X, B, users, items):
    """float32 [n]; a pair with a user or item id out of range scores 0.0."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    ok = (users >= 0) & (users < X.shape[0]) & (items >= 0) & (items < X.shape[1])
    out = np.zeros(len(users), dtype=F32)
    if ok.any():
        out[ok] = _chain(X[users[ok]].astype(F32), np.asarray(B, dtype=F32), items[ok])
    return out


def fit64(X, lam):
    """(A fp32, P* float64, B from P*) of the definition with the float64 inverse."""
    A = matrix(gram(X), lam)
    P, _ = inverse64(A)
    return A, P, weights(P)


# ------------------------------------------------------------------------------------------------------------ the walk
def resolved_block(n, block):
    return int(block) if block else (BLOCKS[0] if n <= BLOCKS[0] else BLOCKS[1])


def gj_unblocked(S):
    """(inverse, None) of a small fp32 matrix by the in-place Gauss-Jordan sweep without pivoting, or (None, p) at the first
    pivot p that is not a finite number > 0."""
    S = np.array(S, dtype=F32)
    for p in range(len(S)):
        piv = S[p, p]
        if not (piv > 0) or not np.isfinite(piv):
            return None, p
        inv = F32(1) / piv
        f = S[:, p].copy()
        row = (S[p] * inv).astype(F32)
        row[p] = inv
        S = (S - np.outer(f, row)).astype(F32)
        S[:, p] = (-f * inv).astype(F32)
        S[p] = row
    return S, None


def invert_walk(A, block=0, variant=None):
    """(P, None), or (None, index of the refused pivot).  variant: None, or one of the wrong sweeps the tests must tell apart:
    "drop_step" leaves one block step out, "touch_pivot_rows" lets the trailing update also subtract from the pivot block-row."""
    A = np.array(A, dtype=F32)
    n = len(A)
    b = resolved_block(n, block)
    for step, k0 in enumerate(range(0, n, b)):
        if variant == "drop_step" and step == min(1, (n - 1) // b):
            continue
        k1 = min(k0 + b, n)
        K, N = np.arange(k0, k1), np.r_[0:k0, k1:n]
        old = A[k0:k1, k0:k1].copy()
        D, bad = gj_unblocked(old)
        if bad is not None:
            return None, k0 + bad
        A[k0:k1, k0:k1] = D
        if not len(N):
            continue
        C = A[np.ix_(N, K)].copy()
        R = (D @ A[np.ix_(K, N)]).astype(F32)
        A[np.ix_(K, N)] = R
        A[np.ix_(N, N)] = (A[np.ix_(N, N)] - C @ R).astype(F32)
        if variant == "touch_pivot_rows":
            A[np.ix_(K, N)] = (R - old @ R).astype(F32)
        A[np.ix_(N, K)] = (-(C @ D)).astype(F32)
    return A, None


# ------------------------------------------------------------------------------------------------------------ budgets
def p_hard(n, kappa, P_star):
    return n * U24 * kappa * float(np.max(np.abs(P_star)))


def p_budget(walk_err, n, kappa, P_star):
    """e_P: what the device may be off by on this input."""
    return min(p_hard(n, kappa, P_star), 4.0 * walk_err + 2.0 * U24 * float(np.max(np.abs(P_star))))


def b_budget(e_P, P_star):
    """e_B [I, I] (float64) from e_P."""
    d = np.diag(P_star)
    assert np.all(d > e_P)
    Bs = np.abs(P_star / d[None, :])
    t = e_P * (1.0 + Bs) / (d[None, :] - e_P)
    e = t + U24 * (Bs + t)
    e[np.arange(len(e)), np.arange(len(e))] = 0.0
    return e


def score_budget(X, users, e_B, P_star):
    """e_S [len(users), I] (float64) from e_B."""
    Q = X[np.asarray(users, dtype=np.int64)].astype(np.float64)
    Bs = np.abs(P_star / np.diag(P_star)[None, :])
    Bs[np.arange(len(Bs)), np.arange(len(Bs))] = 0.0
    n = (Q > 0).sum(axis=1, keepdims=True)
    g = n * U24 / (1.0 - n * U24)
    return Q @ e_B + g * (Q @ (Bs + e_B))


# ------------------------------------------------------------------------------------------------------------ the shared inputs
SIZES = tuple((b, n) for b in BLOCKS for n in (1, 2, 3, b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1, 3 * b + 5)) + ((0, 200), (0, 257))
USERS = (1, 5, 70, 300)
LAMBDAS = (0.5, 10.0, 500.0)


def ratings(U, n, seed, explicit=False):
    """A popularity-skewed U x n matrix of 0/1 (or 1..5) ratings, int64; item n - 2 (when there is one) has no rater."""
    rng = np.random.default_rng(seed)
    pop = 0.6 / (1.0 + np.arange(n)) ** 0.5 + 0.03
    X = (rng.random((U, n)) < pop[None, :]).astype(np.int64)
    if explicit:
        X *= rng.integers(1, 6, size=(U, n))
    if n > 2:
        X[:, n - 2] = 0
    return X


@functools.lru_cache(maxsize=None)
def case(block, n, U, lam, explicit=False):
    """One input of the GPU tests and what is known about it: X, A (fp32), P*, kappa, the walk's P and its error."""
    X = ratings(U, n, 1000 * n + 10 * U + int(explicit), explicit)
    A = matrix(gram(X), lam)
    P_star, kappa = inverse64(A)
    P_walk, bad = invert_walk(A, block)
    assert bad is None
    walk_err = float(np.max(np.abs(P_walk.astype(np.float64) - P_star)))
    for a in (X, A, P_star, P_walk):
        a.setflags(write=False)
    return {"X": X, "A": A, "P_star": P_star, "kappa": kappa, "P_walk": P_walk, "walk_err": walk_err,
            "e_P": p_budget(walk_err, n, kappa, P_star), "e_hard": p_hard(n, kappa, P_star), "max_P": float(np.max(np.abs(P_star)))}


# the inputs of every (block, I): (U, lambda, explicit) with U x lambda crossed on 0/1 ratings, plus one 1..5 case
CASES = tuple((U, lam, False) for U in USERS for lam in LAMBDAS) + ((70, 10.0, True),)


def csr_of(X):
    """(ptr int32, idx int32, val float32) of a dense integer matrix."""
    X = np.asarray(X)
    ptr = np.concatenate([[0], np.cumsum((X != 0).sum(axis=1))]).astype(np.int32)
    r, c = np.nonzero(X)
    return ptr, c.astype(np.int32), X[r, c].astype(np.float32)


def topk_unseen(row, seen, K):
    """Ids of the K best unseen items of one score row: score descending, ties to the lower id."""
    s = np.asarray(row, dtype=np.float64).copy()
    s[np.asarray(seen, dtype=np.int64)] = -np.inf
    order = np.lexsort((np.arange(len(s)), -s))
    return order[: min(K, len(s) - len(seen))]


def hit_ratio(X, lam, target, K, real_users=None):
    """(HR@K of `target` over the users of [0, real_users) who have not rated it, how many such users): the restated model (float64
    inverse) fitted on all of X."""
    _, _, B = fit64(X, lam)
    U = X.shape[0] if real_users is None else real_users
    users = [u for u in range(U) if X[u, target] == 0]
    S = scores(X, B, users)
    hits = sum(target in topk_unseen(S[r], np.nonzero(X[u])[0], K) for r, u in enumerate(users))
    return hits / max(len(users), 1), len(users)
