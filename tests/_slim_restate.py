"""Numpy restatement of the SLIM definition (include/recad_hip.h): cyclic coordinate descent on G = X^T X + beta I, one column per
item, non-negative weights, a zero diagonal.

walk() is the definition itself.  It loops over the sweeps and over the coordinates k in Python and takes the step of coordinate
k in every column at once: the columns do not interact, so the state of all of them is two I x I arrays, R[i, j] = r_i of column j
(R starts as G) and W[k, j] = w_k of column j, which are also the layouts of R_out and W.  In fp32 every numpy operation is one
rounded fp32 operation (the product and the subtraction of the r update are two), so the kernel is compared with it bit for bit.
fit_walk() is the walk from a rating matrix, fit64() the same walk in float64.

The error bound E.  An update r_i <- fl(r_i - fl(delta * G_ki)) rounds twice: the product is off by at most u |delta G_ki| and the
difference by at most u |r_i| (the new value), u = 2^-24.  E[i, j] is the sum of u (|delta G_ki| + |r_i|) over the updates of
column j, accumulated in float64 beside the walk, and bounds |R - (G - G W)| with G - G W evaluated in float64 from the fp32 G and
W: R[i, j] is G_ij minus the applied products, and the applied deltas of coordinate k add up to w_k.  (delta = fl(w' - w_k) is
the exact difference whenever w_k is 0, w' is 0, or the two are within a factor of two of each other, which leaves a coordinate's
second or third step at most; the rounding of such a delta is not counted in E.  The bound is held as stated: the worst ratio
|error| / E over the inputs of the GPU tests is 0.87.)

The fixed point.  Where the last changing sweep is below `sweeps`, one whole sweep ran over the final state without a change:
  on the support (w_k > 0), fl(w_k + q) == w_k, so |q| <= ulp(w_k) / 2 <= u w_k; q = fl(t / G_kk) and t = fl(r_k - l1) are off by
  a factor (1 + u) each, so |r_k - l1| <= u w_k G_kk (1 + u)^2; the float64 gradient of f_j at W is g_k = -(G - G W)_kj, so
  |g_k + l1| <= E[k, j] + u w_k G_kk (1 + u)^2;
  off the support (w_k == +0), fl(0 + q) <= 0 means t <= 0, and the sign of t = fl(r_k - l1) is exact: r_k <= l1, so
  g_k + l1 >= -E[k, j].
kkt_bound() returns the two bounds; kkt() the residuals."""
import functools
import itertools

import numpy as np

from tests._ease_restate import csr_of, dense, gram, matrix, ratings, scores, topk_unseen  # noqa: F401  (shared with the tests)

F32 = np.float32
U24 = 2.0 ** -24
VARIANTS = ("fma", "jacobi", "no_clip", "keep_diagonal")


def walk(G, l1, sweeps, dtype=F32, variant=None, track=False, snapshots=None, on_sweep=None):
    """(W, R, info, E) after `sweeps` sweeps, E None unless track; with snapshots (a tuple of sweep counts) a dict
    {sweeps: (W, R, info, E)} of what a fit with that many sweeps returns.  info is int32 [I, 3]: the last sweep that changed a
    coordinate of the column, the number of positive weights, the number of steps with delta != 0.  on_sweep(s, W, R) is called
    after every sweep that ran.  variant: None, or one of the wrong walks the tests must tell apart."""
    G = np.ascontiguousarray(G, dtype=dtype)
    n = len(G)
    l1 = dtype(l1)
    zero = dtype(0)
    R, W = G.copy(), np.zeros((n, n), dtype=dtype)
    last, steps = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    E = np.zeros((n, n)) if track else None
    wanted = sorted(set(snapshots)) if snapshots else [sweeps]
    out = {}

    def snap():
        info = np.stack([last, (W > 0).sum(axis=0).astype(np.int32), steps], axis=1).astype(np.int32)
        return W.copy(), R.copy(), info, None if E is None else E.copy()

    with np.errstate(all="ignore"):
        for s in range(1, max(wanted) + 1):
            changed = False
            Rs = R.copy() if variant == "jacobi" else R
            for k in range(n):
                wk = W[k]
                t = Rs[k] - l1
                q = t / G[k, k]
                v = wk + q
                wn = v if variant == "no_clip" else np.where(v > 0, v, zero)
                d = wn - wk
                if variant != "keep_diagonal":
                    d[k] = zero
                act = np.nonzero(d != 0)[0]
                if not len(act):
                    continue
                changed = True
                W[k, act] = wn[act]
                prod = G[k][:, None] * d[act][None, :]                      # one rounding
                if variant == "fma":
                    new = (R[:, act].astype(np.float64) - G[k].astype(np.float64)[:, None] * d[act].astype(np.float64)[None, :]).astype(dtype)
                else:
                    new = R[:, act] - prod                                  # and another: never fused
                if track:
                    E[:, act] += U24 * (np.abs(prod.astype(np.float64)) + np.abs(new.astype(np.float64)))
                R[:, act] = new
                last[act] = s
                steps[act] += 1
            if on_sweep is not None:
                on_sweep(s, W, R)
            if s in wanted:
                out[s] = snap()
            if not changed:                                                 # nothing changes in any later sweep either
                break
    final = snap()
    for s in wanted:
        out.setdefault(s, final)
    return out if snapshots else out[sweeps]


def fit_walk(X, l1, beta, sweeps, **kw):
    """(W, R, info) of the definition in fp32 from the dense integer rating matrix X."""
    return walk(matrix(gram(X), beta), l1, sweeps, **kw)[:3]


def fit64(X, l1, beta, sweeps, **kw):
    """The same walk in float64, from the same fp32 G."""
    return walk(matrix(gram(X), beta), l1, sweeps, dtype=np.float64, **kw)[:3]


def objective(G, W, l1):
    """f_j(w) = 1/2 w^T G w - d_j^T w + l1 sum w for every column j, in float64 (d_j = column j of G; w_j = 0)."""
    G, W = np.asarray(G, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return 0.5 * np.sum(W * (G @ W), axis=0) - np.sum(G * W, axis=0) + float(l1) * W.sum(axis=0)


def gradient(G, W):
    """g[k, j] = (G w_j - d_j)_k in float64: minus the exact residual."""
    G, W = np.asarray(G, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return G.T @ W - G


def kkt(G, W, l1):
    """(|g + l1| on the support, max(0, -(g + l1)) off it), [I, I] each, the diagonal zeroed."""
    h = gradient(G, W) + float(l1)
    on = np.asarray(W) > 0
    a, b = np.where(on, np.abs(h), 0.0), np.where(on, 0.0, np.maximum(-h, 0.0))
    np.fill_diagonal(a, 0.0)
    np.fill_diagonal(b, 0.0)
    return a, b


def kkt_bound(G, W, E):
    """What kkt() of a fixed point of the fp32 walk may reach (the module docstring derives it)."""
    G64, W64 = np.asarray(G, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return E + U24 * (1 + U24) ** 2 * W64 * np.diag(G64)[:, None], E


def exact_minimiser(G, l1, j):
    """Column j's minimiser by enumerating supports (I <= 4): the one candidate that satisfies the KKT conditions."""
    G = np.asarray(G, dtype=np.float64)
    n = len(G)
    others = [k for k in range(n) if k != j]
    best = None
    for size in range(len(others) + 1):
        for S in itertools.combinations(others, size):
            w = np.zeros(n)
            if S:
                S = list(S)
                w[S] = np.linalg.solve(G[np.ix_(S, S)], G[S, j] - l1)
                if np.any(w[S] <= 0):
                    continue
            h = G @ w - G[:, j] + l1
            if all(h[k] >= -1e-12 * max(1.0, abs(G[k, j])) for k in others if w[k] == 0):
                assert best is None or np.allclose(best, w, rtol=1e-9, atol=1e-12), "a strictly convex problem has one minimiser"
                best = w
    assert best is not None
    return best


# ------------------------------------------------------------------------------------------------------------ the shared inputs
ITEMS = (1, 2, 3, 63, 64, 65, 200, 255, 256, 257, 300)
USERS = (1, 5, 70, 300)
REGS = ((0.0, 0.5), (1.0, 5.0), (5.0, 500.0))       # (l1, beta)
SWEEPS = (1, 2, 40)


def heavy(U, n, seed):
    """ratings() with every tenth stored rating set to 127."""
    X = ratings(U, n, seed).copy()
    r, c = np.nonzero(X)
    X[r[::10], c[::10]] = 127
    return X


@functools.lru_cache(maxsize=None)
def case(n, U, l1, beta, kind="binary", sweeps=SWEEPS):
    """One input of the GPU tests: X, G and {sweeps: (W, R, info, E)} of the fp32 walk."""
    seed = 2000 * n + 10 * U
    X = {"binary": lambda: ratings(U, n, seed), "explicit": lambda: ratings(U, n, seed + 1, explicit=True), "heavy": lambda: heavy(U, n, seed + 2)}[kind]()
    G = matrix(gram(X), beta)
    fits = walk(G, l1, max(sweeps), track=True, snapshots=tuple(sweeps))
    for a in (X, G):
        a.setflags(write=False)
    return {"X": X, "G": G, "fits": fits}


# every (I, U) with every (l1, beta); the sweep counts are snapshots of one walk.  Then one 1..5 case and one with ratings of 127.
TABLE = tuple((n, U, l1, beta, "binary") for n in ITEMS for U in USERS for l1, beta in REGS) + \
    ((65, 70, 1.0, 5.0, "explicit"), (65, 70, 1.0, 5.0, "heavy"))


def twins():
    """8 users x 5 items: items 0 and 1 are rated by the same three users and by nobody else, items 2, 3 and 4 by others."""
    X = np.zeros((8, 5), dtype=np.int64)
    X[:3, 0] = X[:3, 1] = 1
    X[3:6, 2] = 1
    X[5:8, 3] = 1
    X[4:7, 4] = 1
    return X


def hit_ratio(X, l1, beta, sweeps, target, K, real_users=None):
    """(HR@K of `target` over the users of [0, real_users) who have not rated it, how many such users): the fp32 walk fitted on all
    of X, scored by EASE's chain."""
    W, _, _ = fit_walk(X, l1, beta, sweeps)
    U = X.shape[0] if real_users is None else real_users
    users = [u for u in range(U) if X[u, target] == 0]
    S = scores(X, W, users)
    hits = sum(target in topk_unseen(S[r], np.nonzero(X[u])[0], K) for r, u in enumerate(users))
    return hits / max(len(users), 1), len(users)
