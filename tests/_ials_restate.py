"""Numpy restatement of the iALS victim (include/recad_hip.h, csrc/ials.hip): the float64 definition (gram64, system64, solve64,
sweep64, objective64 over all pairs), a plain fp32 walk (b in the defined order, G and A in a straightforward order, the unblocked
right-looking Cholesky and the column-oriented substitutions, every operation rounded on its own), the budgets, and the fixed case
table the host and GPU tests share.

The budgets, u = 2^-24:
  G   (n + 2) u (|Y|^T |Y| + lambda I) per element: any-order summation of n singly rounded products plus the one add of lambda.
  A   e_G + gamma_{n_u + 1} T + u (|A*| + e_G + gamma_{n_u + 1} T), T = sum_e |w_e y y^T|, gamma_m = m u / (1 - m u): one rounding
      per scaled operand w_e y_ek, one per fma of the chain, one for the add of G (the order csrc/ials.hip chose).
  x   4 x (the fp32 walk's error on the same system) + 2^-23 max|x*|, the project's rule for rk_ease_invert.  As there, the walk
      and the device start from the same fp32 numbers: the GPU tests hand the walk the A_u and b_u that rk_ials_system wrote (its
      own A, summed in another order, can land within a twentieth of an ulp of x* by luck, which no kernel can be held to), and x*
      stays solve64 of the float64 system, so the formation error counts on both sides.
  x, hard.  The computed x solves (A* + E) x = b* + f.  E is the formation error above plus the backward error of the Cholesky
      solve, |E_2| <= gamma_{3d + 1} |L| |L^T| (Higham, Accuracy and Stability, theorem 10.4).  In the 2-norm | |Y|^T |Y| | <=
      |Y|_F^2 = trace(Y^T Y) <= d |A|, likewise |T| <= d |A| and | |L| |L^T| | <= d |A|, so |E| <= u d (n + n_u + 3 d + 6) |A|.
      f is the error of the chain b: |f| <= gamma_{n_u + 1} beta, beta = sum_e c_e |y_e|, which cancellation keeps from being
      bounded by |A| |x| and which therefore stays a term of its own.  With |x|_2 <= sqrt(d) max|x|, and a factor 2 for the
      second-order terms (the caps keep u kappa C far below 1/2):
        max|x - x*| <= 2 u kappa_2(A) [C(d, n_u, n) max|x*| + (n_u + 1) |beta|_2 / |A|_2],  C = d^1.5 (n + n_u + 3 d + 6).
  J   (d + max n_u + 8) 2^-53 relative to the sum of the absolute terms, sum_ui c_ui (p_ui + |x_u| . |y_i|)^2 + lambda (|X|^2 + |Y|^2).
"""
import functools

import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53
CHUNK, GRAM_ROWS, MAX_DIM = 64, 256, 128
KAPPA_CAP, REL_CAP = 2.0 ** 12, 2.0 ** -10
f32 = np.float32


def gamma(m):
    return m * U24 / (1.0 - m * U24)


def confidence(q, alpha):
    """(w, c) in fp32 as defined: w = fl(alpha * (float) q), c = fl(1.0f + w)."""
    w = f32(alpha) * np.asarray(q, dtype=np.float32)
    return w, f32(1.0) + w


# ------------------------------------------------------------------------------------------------------------- float64
def gram64(Y, lam):
    Y = np.asarray(Y, dtype=np.float64)
    return Y.T @ Y + float(f32(lam)) * np.eye(Y.shape[1])


def gram_budget(Y, lam):
    Y = np.abs(np.asarray(Y, dtype=np.float64))
    return (len(Y) + 2) * U24 * (Y.T @ Y + float(f32(lam)) * np.eye(Y.shape[1]))


def system64(G, Y, cols, q, alpha):
    """(A, b) of one row in float64 from the fp32 table and the fp32 confidences."""
    w, c = confidence(q, alpha)
    R = np.asarray(Y, dtype=np.float64)[np.asarray(cols, dtype=np.int64)]
    return np.asarray(G, dtype=np.float64) + (R * w.astype(np.float64)[:, None]).T @ R, (R * c.astype(np.float64)[:, None]).sum(axis=0)


def a_budget(e_G, A_star, Y, cols, q, alpha):
    w, _ = confidence(q, alpha)
    R = np.abs(np.asarray(Y, dtype=np.float64)[np.asarray(cols, dtype=np.int64)])
    T = (R * np.abs(w.astype(np.float64))[:, None]).T @ R
    g = gamma(len(cols) + 1)
    return e_G + g * T + U24 * (np.abs(A_star) + e_G + g * T)


def solve64(A, b):
    return np.linalg.solve(np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64))


def transpose(ptr, idx, val, n_cols):
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    o = np.lexsort((row, idx))
    cptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_cols))]).astype(np.int64)
    return cptr, row[o].astype(np.int64), np.asarray(val)[o]


def half_sweep64(ptr, idx, val, Y, alpha, lam):
    G = gram64(Y, lam)
    X = np.zeros((len(ptr) - 1, Y.shape[1]))
    for u in range(len(ptr) - 1):
        s = slice(ptr[u], ptr[u + 1])
        if ptr[u + 1] > ptr[u]:
            X[u] = solve64(*system64(G, Y, idx[s], val[s], alpha))
    return X


def sweep64(ptr, idx, val, n_cols, Y, alpha, lam):
    """One sweep in float64: (X from Y over the CSR, Y from the new X over the transpose)."""
    X = half_sweep64(ptr, idx, val, np.asarray(Y, dtype=np.float64), alpha, lam)
    return X, half_sweep64(*transpose(ptr, idx, val, n_cols), X, alpha, lam)


def dense(ptr, idx, val, n_cols):
    Q = np.zeros((len(ptr) - 1, n_cols))
    Q[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), idx] = val
    return Q


def objective64(ptr, idx, val, n_cols, X, Y, alpha, lam, absolute=False):
    """J over all U * I pairs in float64, the dense form; absolute: the sum of the absolute terms instead."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    Q = dense(ptr, idx, val, n_cols)
    C = np.where(Q > 0, confidence(Q, alpha)[1].astype(np.float64), 1.0)
    P = (Q > 0).astype(np.float64)
    S = np.abs(X) @ np.abs(Y).T if absolute else X @ Y.T
    res = (P + S) if absolute else (P - S)
    return float(np.sum(C * res * res) + float(f32(lam)) * (np.sum(X * X) + np.sum(Y * Y)))


def objective_rows64(ptr, idx, val, X, Y, alpha, lam):
    """The same J without the dense matrix, as the device evaluates it: per row x^T (Y^T Y) x + sum_e [c_e (1 - s_e)^2 - s_e^2] +
    lambda |x|^2, and lambda |Y|^2 once.  Returns (J, the per-row doubles)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    GY, lam = Y.T @ Y, float(f32(lam))
    rows = np.zeros(len(X))
    for u in range(len(X)):
        s = slice(ptr[u], ptr[u + 1])
        c = confidence(val[s], alpha)[1].astype(np.float64)
        dots = Y[idx[s]] @ X[u]
        rows[u] = X[u] @ GY @ X[u] + np.sum(c * (1.0 - dots) ** 2 - dots ** 2) + lam * (X[u] @ X[u])
    return float(rows.sum() + lam * np.trace(GY)), rows


def j_budget(ptr, idx, val, n_cols, X, Y, alpha, lam):
    n_max = int(np.max(np.diff(ptr))) if len(ptr) > 1 else 0
    return (X.shape[1] + n_max + 8) * U53 * objective64(ptr, idx, val, n_cols, X, Y, alpha, lam, absolute=True)


# ------------------------------------------------------------------------------------------------------- the fp32 walk
def gram_walk(Y, lam):
    Y = np.asarray(Y, dtype=np.float32)
    G = np.zeros((Y.shape[1], Y.shape[1]), dtype=np.float32)
    for y in Y:
        G += y[:, None] * y[None, :]
    return G + f32(lam) * np.eye(Y.shape[1], dtype=np.float32)


def b_walk(Y, cols, q, alpha):
    """b_u as defined: s_0 = +0.0f, s_{e+1} = s_e + fl(c_e * y_{i_e}); bit-exact."""
    Y = np.asarray(Y, dtype=np.float32)
    _, c = confidence(q, alpha)
    s = np.zeros(Y.shape[1], dtype=np.float32)
    for e, i in enumerate(cols):
        s = s + c[e] * Y[i]
    return s


def system_walk(G32, Y, cols, q, alpha):
    Y = np.asarray(Y, dtype=np.float32)
    w, _ = confidence(q, alpha)
    t = np.zeros_like(G32)
    for e, i in enumerate(cols):
        t = t + (w[e] * Y[i])[:, None] * Y[i][None, :]
    return G32 + t, b_walk(Y, cols, q, alpha)


def cholesky_walk(A):
    """(L, None), or (None, p) at the first pivot that is not a finite number > 0.  Right-looking, a column at a time."""
    A = np.array(A, dtype=np.float32)
    d = len(A)
    for p in range(d):
        piv = A[p, p]
        if not (piv > 0 and np.isfinite(piv)):
            return None, p
        r = np.sqrt(piv)
        A[p, p] = r
        A[p + 1:, p] = A[p + 1:, p] / r
        col = A[p + 1:, p]
        A[p + 1:, p + 1:] = A[p + 1:, p + 1:] - col[:, None] * col[None, :]
    return np.tril(A), None


def solve_walk(A, b, transposed_solve=False):
    """x in fp32 by the walk, or None when the factorisation is refused.  transposed_solve: the defect the host test plants (the
    forward substitution run on L^T)."""
    L, bad = cholesky_walk(A)
    if L is None:
        return None
    d = len(L)
    v = np.array(b, dtype=np.float32)
    F = L.T.copy() if transposed_solve else L
    for p in range(d):
        v[p] = v[p] / F[p, p]
        v[p + 1:] = v[p + 1:] - F[p + 1:, p] * v[p]
    for p in range(d - 1, -1, -1):
        v[p] = v[p] / L[p, p]
        v[:p] = v[:p] - L[p, :p] * v[p]
    return v


def b_budget(Y, cols, q, alpha):
    """gamma_{n_u + 1} sum_e c_e |y_e| per component: one rounding per product, one per add."""
    _, c = confidence(q, alpha)
    return gamma(len(cols) + 1) * (np.abs(np.asarray(Y, dtype=np.float64)[np.asarray(cols, dtype=np.int64)]) * c.astype(np.float64)[:, None]).sum(axis=0)


def x_budget(walk_err, x_star):
    return 4.0 * walk_err + 2.0 ** -23 * float(np.max(np.abs(x_star), initial=0.0))


def c_hard(d, n_u, n):
    return d ** 1.5 * (n + n_u + 3 * d + 6)


def x_hard(A_star, x_star, Y, cols, q, alpha, n):
    d, n_u = len(A_star), len(cols)
    ev = np.linalg.eigvalsh(A_star)
    _, c = confidence(q, alpha)
    beta = (np.abs(np.asarray(Y, dtype=np.float64)[np.asarray(cols, dtype=np.int64)]) * c.astype(np.float64)[:, None]).sum(axis=0)
    kappa = float(ev[-1] / ev[0])
    return kappa, 2.0 * U24 * kappa * (c_hard(d, n_u, n) * float(np.max(np.abs(x_star), initial=0.0))
                                      + (n_u + 1) * float(np.linalg.norm(beta)) / float(ev[-1]))


# ------------------------------------------------------------------------------------------------------- the case table
DIMS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 127, 128)
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
SIZES = (1, 7, 70, 300, GRAM_ROWS - 1, GRAM_ROWS, GRAM_ROWS + 1, 2 * GRAM_ROWS + 5)
ALPHA_LAMBDA = ((0.0, 0.5), (1.0, 0.5), (40.0, 10.0))
RATINGS = ("ones", "1..5")
STATES = ("init", "swept")


def _table():
    cases = []
    for i, d in enumerate(DIMS):
        for j, n in enumerate(SIZES):
            al = ALPHA_LAMBDA[(i + j) % 3]
            cases.append((d, n, al[0], al[1], RATINGS[(i + 2 * j + (i + j) // 3) % 2], STATES[(i // 2 + j) % 2]))
    cases.append((32, 300, 1.0, 64.0, "127", "swept"))          # the one case at the largest rating
    return tuple(cases)


CASES = _table()


def case_id(c):
    return f"d{c[0]}-n{c[1]}-a{c[2]:g}-l{c[3]:g}-{c[4]}-{c[5]}"


def small_cases(limit=70):
    """The cases whose dense objective is cheap: the other side's size at most `limit`."""
    return tuple(c for c in CASES if c[1] <= limit)


@functools.lru_cache(maxsize=None)
def case(c):
    """Everything known without the device about one case: the CSR (one row per length that fits n), the fp32 table, G, and per
    row the float64 system, its solution, the walk's error and the budgets."""
    d, n, alpha, lam, ratings, state = c
    rng = np.random.default_rng(7919 * CASES.index(c) + 13)
    lens = sorted({min(L, n) for L in ROW_LENGTHS})
    rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    nnz = len(idx)
    val = {"ones": np.ones(nnz), "1..5": rng.integers(1, 6, size=nnz), "127": np.full(nnz, 127)}[ratings].astype(np.float32)
    Y = (0.01 * rng.standard_normal((n, d))).astype(np.float32)
    if state == "swept":
        Y64 = Y.astype(np.float64)
        for _ in range(2):
            _, Y64 = sweep64(ptr, idx, val, n, Y64, alpha, lam)
        Y = Y64.astype(np.float32)
    G64, e_G, G32 = gram64(Y, lam), gram_budget(Y, lam), gram_walk(Y, lam)
    out = {"d": d, "n": n, "alpha": alpha, "lam": lam, "ptr": ptr, "idx": idx, "val": val, "Y": Y, "G64": G64, "e_G": e_G, "G32": G32,
           "rows": []}
    for u, L in enumerate(lens):
        s = slice(ptr[u], ptr[u + 1])
        A, b = system64(G64, Y, idx[s], val[s], alpha)
        x = solve64(A, b)
        Aw, bw = system_walk(G32, Y, idx[s], val[s], alpha)
        xw = solve_walk(Aw, bw)
        kappa, hard = x_hard(A, x, Y, idx[s], val[s], alpha, n)
        walk_err = float(np.max(np.abs(xw.astype(np.float64) - x))) if xw is not None else float("inf")
        out["rows"].append({"A": A, "b": b, "x": x, "e_A": a_budget(e_G, A, Y, idx[s], val[s], alpha), "b_walk": bw, "A_walk": Aw,
                            "e_b": b_budget(Y, idx[s], val[s], alpha),
                            "kappa": kappa, "walk_err": walk_err, "e_x": x_budget(walk_err, x), "e_hard": hard, "n_u": L})
    return out


# ------------------------------------------------------------------------------------------------------- the push attack
def scores64(X, Y):
    return np.asarray(X, dtype=np.float64) @ np.asarray(Y, dtype=np.float64).T


def fit64(ptr, idx, val, n_cols, Y0, alpha, lam, sweeps):
    Y = np.asarray(Y0, dtype=np.float64)
    for _ in range(sweeps):
        X, Y = sweep64(ptr, idx, val, n_cols, Y, alpha, lam)
    return X, Y


def hit_ratio(S, ptr, idx, target, k, real_users=None):
    """HR@k of `target` over the users (the first real_users rows) who have not rated it; seen items are excluded from the list."""
    n_users = len(ptr) - 1 if real_users is None else real_users
    hits = n = 0
    for u in range(n_users):
        seen = idx[ptr[u]:ptr[u + 1]]
        if target in seen:
            continue
        row = np.array(S[u], dtype=np.float64)
        row[seen] = -np.inf
        hits += int(np.sum(row > row[target]) < k)
        n += 1
    return hits / max(n, 1), n


def half_sweep_walk(ptr, idx, val, Y, alpha, lam):
    """One half-sweep by the fp32 walk (every row, the empty ones too)."""
    Y = np.asarray(Y, dtype=np.float32)
    G = gram_walk(Y, lam)
    X = np.zeros((len(ptr) - 1, Y.shape[1]), dtype=np.float32)
    for u in range(len(ptr) - 1):
        s = slice(ptr[u], ptr[u + 1])
        X[u] = solve_walk(*system_walk(G, Y, idx[s], val[s], alpha))
    return X


def fit_walk(ptr, idx, val, n_cols, Y0, alpha, lam, sweeps):
    Y = np.asarray(Y0, dtype=np.float32)
    tp = transpose(ptr, idx, val, n_cols)
    for _ in range(sweeps):
        X = half_sweep_walk(ptr, idx, val, Y, alpha, lam)
        Y = half_sweep_walk(*tp, X, alpha, lam)
    return X, Y
