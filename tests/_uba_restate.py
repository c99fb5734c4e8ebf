"""NumPy float64 restatement of UBA's target-user selection up to prob_mat (recad/model/attacker/uba.py:81-140), the oracle of
csrc/uba.hip: the redraw from given draws, the score rows in both modes, the counts and prob_mat.  The matrix mode is written
the literal way -- the redrawn train matrix with its appended rows, the expanded (M+N)^2 matrix, ``@`` twice -- and a second
time as the weighted sum the kernels use, so that the identity between the two is a test and not an assumption.  Every value
is an integer below 2^53, so float64 is exact here and comparisons are equalities."""
import numpy as np

TRIALS, TOPN = 10, 10


def dense(n_users, n_items, ptr, idx, val):
    m = np.zeros((n_users, n_items), dtype=np.float64)
    rows = np.repeat(np.arange(n_users), np.diff(ptr))
    m[rows, idx] = val
    return m


def side_layout(mat, targets, s):
    """(side_ptr, side_col): per target user the rated items ascending, with s in its place whether rated or not."""
    cols = [np.union1d(np.nonzero(mat[u])[0], [s]) for u in targets]
    ptr = np.zeros(len(targets) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(c) for c in cols])
    return ptr, np.concatenate(cols).astype(np.int64)


def redraw(mat, targets, s, draws):
    """uba.py:86-91 on a copy: draws [side_ptr[-1]] in side layout (the entry at s is ignored).  Returns (the redrawn matrix,
    side_val)."""
    ptr, col = side_layout(mat, targets, s)
    val = np.asarray(draws, dtype=np.float64).copy()
    val[col == s] = 5.0
    out = np.array(mat, dtype=np.float64)
    for t, u in enumerate(targets):
        out[u, col[ptr[t]:ptr[t + 1]]] = val[ptr[t]:ptr[t + 1]]
    return out, val.astype(np.int64)


def scores_elementwise(redrawn, targets):
    """uba.py:99 as written: the elementwise cube of the expanded matrix, rows target_user_ids of its upper right block."""
    r = redrawn[list(targets)]
    return r * r * r


def scores_matrix_literal(redrawn, targets, b):
    """uba.py:92-101 with ``@`` for ``*``: b copies of each redrawn target row appended, the expanded (M+N)^2 matrix built as the
    reference builds it, cubed as a matrix."""
    train = redrawn
    for u in targets:
        for _ in range(b):
            train = np.vstack([train, redrawn[u]])
    M, N = train.shape
    E = np.zeros((M + N, M + N))
    E[:M, M:M + N] = train
    E[M:M + N, :M] = train.T
    A3 = (E @ E @ E)[:M, M:M + N]
    return A3[list(targets), :]


def scores_matrix_weighted(redrawn, targets, b, target_weight=None):
    """x_t = sum_v c_v <r'_v, r'_t> r'_v with c_v = 1 + b for a target user, 1 otherwise (target_weight overrides 1 + b: the
    tests use it to show that a wrong weight is caught)."""
    c = np.ones(redrawn.shape[0])
    c[list(targets)] = 1 + b if target_weight is None else target_weight
    w = (redrawn @ redrawn[list(targets)].T) * c[:, None]           # [n_users, n_targets]
    return w.T @ redrawn


def counts(x, s):
    """(n_greater, n_equal, n_equal_before) per row of x against x[:, s]."""
    xs = x[:, s:s + 1]
    eq = x == xs
    eq[:, s] = False
    return (x > xs).sum(axis=1), eq.sum(axis=1), eq[:, :s].sum(axis=1)


def hit_and_tie(x, s):
    g, e, eb = counts(x, s)
    return g + eb < TOPN, (g < TOPN) & (g + e >= TOPN)


def prob(mat, targets, s, budget, draws, mode, score=None):
    """budget_matrix (uba.py:119-140) on draws [budget, TRIALS, side_ptr[-1]]: (prob_mat [n_targets, budget], the number of
    tie-dependent cases, hits [budget, TRIALS, n_targets] bool, ties alike)."""
    n = len(targets)
    hits = np.zeros((budget, TRIALS, n), dtype=bool)
    ties = np.zeros((budget, TRIALS, n), dtype=bool)
    for b in range(1, budget + 1):
        for trial in range(TRIALS):
            red, _ = redraw(mat, targets, s, draws[b - 1, trial])
            if score is not None:
                x = score(red, targets, b)
            elif mode == "elementwise":
                x = scores_elementwise(red, targets)
            else:
                x = scores_matrix_weighted(red, targets, b)
            hits[b - 1, trial], ties[b - 1, trial] = hit_and_tie(x, s)
    return hits.sum(axis=1).T / float(TRIALS), int(ties.sum()), hits, ties
