"""Numpy restatement of the PGA attacker (include/recad_hip.h, csrc/pga.hip), stage by stage from each stage's own inputs: the
loss terms and D, g, Z, M, h, V, grad in float64, their budgets, plain fp32 forms in two summation orders, the exact fp32 walks
where the order is fixed (the update, max|grad|, the selection, the sparse sums of h, the Cholesky solve with a given
right-hand side through tests/_ials_restate.py), the relaxed sweep in torch float64 the closed form is held to, and the case
table the host and GPU tests share.

The budgets, u = 2^-24, gamma_m = m u / (1 - m u); every one is a count of roundings times the sum of the absolute terms:
  terms, D   the device works in double from the fp32 scores and rounds D once: u |D*| + 2^-44 / |E_t| per element, and
             2^-44 (|lse| + |s_t| + 1) / |E_t| per loss term (libm's exp and log in double, the lane-strided sum).
  g          gamma_{n + p + 1} (|D|^T |X|), n the users times the targets, p the partial products: any-order summation of n
             singly rounded products and the p adds of the parts.
  M          gamma_{I + 1} (|Z|^T |Y+|).
  h          the device sums cf_j z_j - wbar q_j y+_j with cf_j = 1 + wbar (1 - s+_j) formed first ((1 + wbar) z - wbar s+ z cancels
             to one part in wbar on a fitted entry, where s+ is near 1): gamma_{n_f + 6} sparse + gamma_{d + 4} dense +
             gamma_{d + 3} amplified, sparse = sum_j [|cf_j| |z_j| + wbar |q_j| |y+_j|] (three roundings a term, the running
             sum over n_f entries, the last subtraction), dense = (|M| + |M|^T) |x| (the add, the product, the l-ordered sum, the
             last subtraction), amplified = wbar sum_j [(|x| . |y+_j| + 1) |z_j| + (|x| . |z_j|) |y+_j|]:
             the errors of the dots s+_j and q_j and of 1 - s+_j, which reach h times wbar |z_j| and wbar |y+_j|.
  grad       gamma_{d + 8} main + gamma_{d + 3} amplified in the same way, per element: main = |1 + wbar (1 - s+)| (|x| . |z|) +
             |1 + wbar (1 - so)| (|yo| . |v|), amplified = wbar [(|x| . |y+| + 1)(|x| . |z|) + (|x| . |yo| + 1)(|yo| . |v|)].
  Z, V       the rule of rk_ials_half_sweep: 4 x (the fp32 walk's error on the system the device built) + 2^-23 max|x*|, and
             the hard bound 2 u kappa_2(A) d^1.5 (n + n_u + 3 d + 6) max|x*| (tests/_ials_restate.py with an exact right-hand
             side: f = 0).
The update, the pinning, max|grad| and the selection are exact."""
import functools

import numpy as np

from . import _ials_restate as IR

U24, U53 = IR.U24, IR.U53
REL_CAP, KAPPA_CAP = IR.REL_CAP, IR.KAPPA_CAP
f32 = np.float32
gamma = IR.gamma


def wbar32(alpha, rating):
    return f32(alpha) * f32(rating)


# ------------------------------------------------------------------------------------------------------------- the data
def fake_csr(cols, rating):
    """(ptr, idx, val) of the binarised rows: cols [A, len] ascending per row."""
    cols = np.asarray(cols, dtype=np.int64)
    A, ln = cols.shape
    return np.arange(A + 1, dtype=np.int64) * ln, cols.reshape(-1), np.full(A * ln, rating, dtype=np.float32)


def combined_csr(ptr, idx, val, cols, rating):
    fp, fi, fv = fake_csr(cols, rating)
    return (np.concatenate([ptr, ptr[-1] + fp[1:]]).astype(np.int64), np.concatenate([idx, fi]).astype(np.int64),
            np.concatenate([val, fv]).astype(np.float32))


def eligible(ptr, idx, n_users, target):
    e = np.ones(n_users, dtype=bool)
    e[np.repeat(np.arange(n_users), np.diff(ptr))[np.asarray(idx) == target]] = False
    return e


# ------------------------------------------------------------------------------------------------------------- float64
def loss_stage64(S, ptr, idx, u0, target, elig, inv, defect=None):
    """(D [nb, I] float64, terms [nb]) from a block of scores (row b: user u0 + b).  defect: 'no_mask', 'no_inv'."""
    S = np.asarray(S, dtype=np.float64)
    D, terms = np.zeros_like(S), np.zeros(len(S))
    scale = 1.0 if defect == "no_inv" else inv
    for b in range(len(S)):
        u = u0 + b
        if not elig[u]:
            continue
        mask = np.ones(S.shape[1], dtype=bool)
        if defect != "no_mask":
            mask[idx[ptr[u]:ptr[u + 1]]] = False
        m = S[b][mask].max()
        lse = m + np.log(np.sum(np.exp(S[b][mask] - m)))
        p = np.where(mask, np.exp(S[b] - lse), 0.0)
        p[target] -= 1.0
        D[b] = p * scale
        terms[b] = (lse - S[b, target]) * scale
    return D, terms


def d_budget(D64, inv):
    return U24 * np.abs(D64) + 2.0 ** -44 * inv


def term_budget(S, target, terms, inv):
    S = np.asarray(S, dtype=np.float64)
    return 2.0 ** -44 * (np.abs(terms) / inv + 2.0 * np.abs(S[:, target]) + 1.0) * inv


def g_stage64(D_blocks, X_blocks):
    return sum(np.asarray(D, dtype=np.float64).T @ np.asarray(X, dtype=np.float64) for D, X in zip(D_blocks, X_blocks))


def g_budget(D_blocks, X_blocks):
    n = sum(len(D) for D in D_blocks)
    return gamma(n + len(D_blocks) + 1) * sum(np.abs(np.asarray(D, np.float64)).T @ np.abs(np.asarray(X, np.float64)) for D, X in zip(D_blocks, X_blocks))


def solve_stage64(Y, lam, ptr, idx, val, alpha, rhs, rows=None):
    """x_u = A_u^-1 rhs_u in float64 for the rows asked (all by default): A_u from the fp32 table as IR.system64 forms it."""
    G = IR.gram64(Y, lam)
    rows = range(len(ptr) - 1) if rows is None else rows
    out = np.zeros((len(rows), np.asarray(Y).shape[1]))
    for k, u in enumerate(rows):
        s = slice(ptr[u], ptr[u + 1])
        A, _ = IR.system64(G, Y, idx[s], val[s], alpha)
        out[k] = IR.solve64(A, np.asarray(rhs, dtype=np.float64)[u])
    return out


def m_stage64(Z, Yp):
    return np.asarray(Z, dtype=np.float64).T @ np.asarray(Yp, dtype=np.float64)


def m_budget(Z, Yp):
    return gamma(len(Z) + 1) * (np.abs(np.asarray(Z, np.float64)).T @ np.abs(np.asarray(Yp, np.float64)))


def h_stage64(Z, Yp, Xf, M, cols, wbar, absolute=False, defect=None):
    """h_f for every fake row.  defect: 'no_mt' (M^T left out), 'w_for_c' (wbar where 1 + wbar belongs)."""
    Z, Yp, Xf, M = (np.asarray(a, dtype=np.float64) for a in (Z, Yp, Xf, M))
    w = float(wbar)
    c1 = w if defect == "w_for_c" else 1.0 + w
    if absolute:
        Z, Yp, Xf, M = np.abs(Z), np.abs(Yp), np.abs(Xf), np.abs(M)
    sgn = 1.0 if absolute else -1.0
    H = np.zeros_like(Xf)
    for f, x in enumerate(Xf):
        zs, ys = Z[cols[f]], Yp[cols[f]]
        sym = M if defect == "no_mt" else M + M.T
        H[f] = c1 * zs.sum(axis=0) + sgn * (sym @ x) + sgn * w * (((ys @ x)[:, None] * zs).sum(axis=0) + ((zs @ x)[:, None] * ys).sum(axis=0))
    return H


def h_budget(Z, Yp, Xf, M, cols, wbar):
    """The device forms cf_j = 1 + wbar (1 - s+_j) first, so what is summed is cf_j z_j - wbar q_j y+_j and (M + M^T) x; the
    error of the dot s+_j reaches h amplified by wbar |z_j|, a term of its own."""
    Z, Yp, Xf, M = (np.asarray(a, dtype=np.float64) for a in (Z, Yp, Xf, M))
    d, n_f, w = Xf.shape[1], np.asarray(cols).shape[1], float(wbar)
    out = np.zeros_like(Xf)
    for f, x in enumerate(Xf):
        zs, ys = Z[cols[f]], Yp[cols[f]]
        cf = 1.0 + w * (1.0 - ys @ x)
        sparse = (np.abs(cf)[:, None] * np.abs(zs)).sum(axis=0) + w * (np.abs(zs @ x)[:, None] * np.abs(ys)).sum(axis=0)
        dense = (np.abs(M) + np.abs(M).T) @ np.abs(x)
        amplified = w * ((np.abs(ys) @ np.abs(x) + 1.0)[:, None] * np.abs(zs) + (np.abs(zs) @ np.abs(x))[:, None] * np.abs(ys)).sum(axis=0)
        out[f] = gamma(n_f + 6) * sparse + gamma(d + 4) * dense + gamma(d + 3) * amplified
    return out


def grad_stage64(Xf, V, Z, Yp, Yo, wbar, absolute=False, defect=None):
    """grad [A, I].  defect: 'no_yo' (the Yo term dropped), 'so_for_sp', 'w_for_c'."""
    Xf, V, Z, Yp, Yo = (np.asarray(a, dtype=np.float64) for a in (Xf, V, Z, Yp, Yo))
    w = float(wbar)
    c1 = w if defect == "w_for_c" else 1.0 + w
    if absolute:
        Xf, V, Z, Yp, Yo = np.abs(Xf), np.abs(V), np.abs(Z), np.abs(Yp), np.abs(Yo)
    sgn = 1.0 if absolute else -1.0
    a, sp, so, b = Xf @ Z.T, Xf @ Yp.T, Xf @ Yo.T, V @ Yo.T
    if defect == "so_for_sp":
        sp = so
    return (c1 + sgn * w * sp) * a + (0.0 if defect == "no_yo" else (c1 + sgn * w * so) * b)


def grad_budget(Xf, V, Z, Yp, Yo, wbar):
    """As h_budget: the coefficients 1 + wbar (1 - s) are formed first; a dot's error reaches grad amplified by wbar."""
    Xf, V, Z, Yp, Yo = (np.asarray(a, dtype=np.float64) for a in (Xf, V, Z, Yp, Yo))
    d, w = Xf.shape[1], float(wbar)
    aX, aV, aZ, aP, aO = np.abs(Xf), np.abs(V), np.abs(Z), np.abs(Yp), np.abs(Yo)
    a_abs, b_abs = aX @ aZ.T, aV @ aO.T
    main = np.abs(1.0 + w * (1.0 - Xf @ Yp.T)) * a_abs + np.abs(1.0 + w * (1.0 - Xf @ Yo.T)) * b_abs
    amplified = w * ((aX @ aP.T + 1.0) * a_abs + (aX @ aO.T + 1.0) * b_abs)
    return gamma(d + 8) * main + gamma(d + 3) * amplified


def hard_rhs(A_star, x_star, n_u, n):
    """(kappa_2, the hard bound) of a solve with an exact right-hand side."""
    ev = np.linalg.eigvalsh(A_star)
    kappa = float(ev[-1] / ev[0])
    return kappa, 2.0 * U24 * kappa * IR.c_hard(len(A_star), n_u, n) * float(np.max(np.abs(x_star), initial=0.0))


# ------------------------------------------------------------------------------------------------- plain fp32, two orders
def _flip(a, axis, order):
    return np.flip(a, axis=axis) if order else a


def g_f32(D_blocks, X_blocks, order):
    out = np.zeros((np.asarray(D_blocks[0]).shape[1], np.asarray(X_blocks[0]).shape[1]), dtype=np.float32)
    for D, X in (zip(D_blocks, X_blocks) if not order else zip(D_blocks[::-1], X_blocks[::-1])):
        out = out + _flip(np.asarray(D, np.float32), 0, order).T @ _flip(np.asarray(X, np.float32), 0, order)
    return out


def m_f32(Z, Yp, order):
    return _flip(np.asarray(Z, np.float32), 0, order).T @ _flip(np.asarray(Yp, np.float32), 0, order)


def h_f32(Z, Yp, Xf, M, cols, wbar, order):
    Z, Yp, Xf, M = (np.asarray(a, dtype=np.float32) for a in (Z, Yp, Xf, M))
    w, one = f32(wbar), f32(1.0)
    H = np.zeros_like(Xf)
    for f, x in enumerate(Xf):
        cs = np.asarray(cols[f])[::-1] if order else np.asarray(cols[f])
        zs, ys = Z[cs], Yp[cs]
        cf = one + w * (one - ys @ x)
        H[f] = (cf[:, None] * zs - (w * (zs @ x))[:, None] * ys).sum(axis=0) - (M + M.T) @ x
    return H


def grad_f32(Xf, V, Z, Yp, Yo, wbar, order):
    Xf, V, Z, Yp, Yo = (_flip(np.asarray(a, dtype=np.float32), 1, order) for a in (Xf, V, Z, Yp, Yo))
    w, one = f32(wbar), f32(1.0)
    return (one + w * (one - Xf @ Yp.T)) * (Xf @ Z.T) + (one + w * (one - Xf @ Yo.T)) * (V @ Yo.T)


# ------------------------------------------------------------------------------------------------------- the fp32 walks
def h_walk(Z, Yp, M, x, sp, q, cols_f, wbar):
    """h of one fake row as csrc/pga.hip adds it, from the row's dots sp = x . y+_j and q = x . z_j (whose order inside a wave
    is the butterfly's): cf = 1 + wbar (1 - sp), t += fl(cf z_j) - fl(fl(wbar q) y+_j) in column order, h = t - m, m the l-ordered
    sum of fl(M_kl + M_lk) x_l; every operation rounded on its own."""
    Z, Yp, M, x = (np.asarray(a, dtype=np.float32) for a in (Z, Yp, M, x))
    w, one = f32(wbar), f32(1.0)
    t = np.zeros(Z.shape[1], dtype=np.float32)
    for e, j in enumerate(cols_f):
        cf = one + w * (one - f32(sp[e]))
        t = t + (cf * Z[j] - (w * f32(q[e])) * Yp[j])
    m = np.zeros(len(x), dtype=np.float32)
    for l in range(len(x)):
        m = m + (M[:, l] + M[l, :]) * x[l]
    return t - m


def max_abs_bits(grad):
    return int(np.abs(np.asarray(grad, dtype=np.float32)).view(np.uint32).max())


def update_walk(R, grad, gmax_bits, lr, targets, pin=True):
    """R after the update and the pinning, bit for bit: q = fl(g / m), st = fl(lr q), v = fl(R - st), clipped; m = 0: no update."""
    R = np.array(R, dtype=np.float32)
    if gmax_bits:
        gm = np.array([gmax_bits], dtype=np.uint32).view(np.float32)[0]
        v = R - f32(lr) * (np.asarray(grad, dtype=np.float32) / gm)
        R = np.where(v > 0, np.minimum(v, f32(1.0)), f32(0.0)).astype(np.float32)
    if pin:
        R[:, list(targets)] = 1.0
    return R


def select_row(r, targets, filler_num, ties="low"):
    """The targets and the filler_num non-targets of largest strength (ties to the lower id), ascending."""
    ids = np.setdiff1d(np.arange(len(r)), np.asarray(targets))
    tie = ids if ties == "low" else -ids
    pick = ids[np.lexsort((tie, -np.asarray(r, dtype=np.float64)[ids]))][:filler_num]
    return np.sort(np.concatenate([np.asarray(targets, dtype=np.int64), pick]))


def select(R, targets, filler_num, ties="low"):
    return np.stack([select_row(r, targets, filler_num, ties) for r in R])


# ------------------------------------------------------------------------------------------------------- the chain
def chain64(ptr, idx, val, n_items, cols, Yo, targets, alpha, lam, rating, defect=None):
    """Everything in float64 from the data, the profiles and Yo: X, Yp, the loss, g, Z, M, H, V, grad."""
    U = len(ptr) - 1
    wbar = float(wbar32(alpha, rating))
    cp, ci, cv = combined_csr(ptr, idx, val, cols, rating)
    Yo = np.asarray(Yo, dtype=np.float64)
    X = IR.half_sweep64(cp, ci, cv, Yo, alpha, lam)
    tp = IR.transpose(cp, ci, cv, n_items)
    Yp = IR.half_sweep64(*tp, X, alpha, lam)
    S = X[:U] @ Yp.T
    loss, Ds = 0.0, []
    for t in targets:
        e = eligible(ptr, idx, U, t)
        D, terms = loss_stage64(S, ptr, idx, 0, t, e, 1.0 / e.sum(), defect=defect)
        loss += terms.sum()
        Ds.append(D)
    g = g_stage64(Ds, [X[:U]] * len(Ds))
    Z = solve_stage64(X, lam, *tp, alpha, g)
    M = m_stage64(Z, Yp)
    H = h_stage64(Z, Yp, X[U:], M, cols, wbar, defect=defect)
    V = solve_stage64(Yo, lam, *fake_csr(cols, rating), alpha, H)
    grad = grad_stage64(X[U:], V, Z, Yp, Yo, wbar, defect=defect)
    return {"X": X, "Yp": Yp, "loss": loss, "D": Ds, "g": g, "Z": Z, "M": M, "H": H, "V": V, "grad": grad}


def relaxed_loss_torch(ptr, idx, val, n_items, R, Yo, targets, alpha, lam, rating):
    """L(Y+(X(R), R)) under the linear relaxation, as a torch float64 graph through torch.linalg.solve: R [A, I] is the leaf."""
    import torch

    U, d = len(ptr) - 1, np.asarray(Yo).shape[1]
    w, lam = float(wbar32(alpha, rating)), float(f32(lam))
    Yo64 = np.asarray(Yo, dtype=np.float64)
    Xr = torch.from_numpy(IR.half_sweep64(ptr, idx, val, Yo64, alpha, lam))          # the real rows do not depend on R
    Q = IR.dense(ptr, idx, val, n_items)
    Wr = torch.from_numpy(np.where(Q > 0, IR.confidence(Q, alpha)[0].astype(np.float64), 0.0))
    Cr = torch.from_numpy(np.where(Q > 0, IR.confidence(Q, alpha)[1].astype(np.float64), 0.0))
    Y = torch.from_numpy(Yo64)
    eye = torch.eye(d, dtype=torch.float64)
    Go = Y.T @ Y + lam * eye
    Af = Go[None] + torch.einsum("fj,jk,jl->fkl", w * R, Y, Y)
    Xf = torch.linalg.solve(Af, ((1.0 + w) * R @ Y)[:, :, None])[:, :, 0]
    X = torch.cat([Xr, Xf])
    Wall = torch.cat([Wr, w * R])                                                     # [U + A, I]
    B = (X.T @ X + lam * eye)[None] + torch.einsum("uj,uk,ul->jkl", Wall, X, X)
    b = torch.cat([Cr, (1.0 + w) * R]).T @ X
    Yp = torch.linalg.solve(B, b[:, :, None])[:, :, 0]
    S = Xr @ Yp.T
    rated = torch.from_numpy(Q > 0)
    Sm = S.masked_fill(rated, float("-inf"))
    lse = torch.logsumexp(Sm, dim=1)
    loss = 0.0
    for t in targets:
        e = torch.from_numpy(eligible(ptr, idx, U, t))
        loss = loss + ((lse - S[:, t])[e]).sum() / float(e.sum())
    return loss


def binary_R(cols, n_items):
    R = np.zeros((len(cols), n_items))
    np.put_along_axis(R, np.asarray(cols, dtype=np.int64), 1.0, axis=1)
    return R


def iterate64(ptr, idx, val, n_items, R0, targets, filler_num, Y0, alpha, lam, rating, lr, init_sweeps, sweeps, iters):
    """The whole attacker in float64: iters train_steps from R0 and the seeded table Y0 -> (R, profiles, losses)."""
    R, Y, losses = np.array(R0, dtype=np.float64), np.asarray(Y0, dtype=np.float64), []
    R[:, list(targets)] = 1.0
    for it in range(iters):
        cols = select(R, targets, filler_num)
        cp, ci, cv = combined_csr(ptr, idx, val, cols, rating)
        for _ in range((init_sweeps if it == 0 else sweeps) - 1):
            _, Y = IR.sweep64(cp, ci, cv, n_items, Y, alpha, lam)
        ch = chain64(ptr, idx, val, n_items, cols, Y, targets, alpha, lam, rating)
        Y = ch["Yp"]
        losses.append(ch["loss"])
        m = np.abs(ch["grad"]).max()
        if m > 0:
            R = np.clip(R - lr * ch["grad"] / m, 0.0, 1.0)
        R[:, list(targets)] = 1.0
    return R, select(R, targets, filler_num), losses


# ------------------------------------------------------------------------------------------------------- the case table
# d, I, U, A, filler_num, n_targets, alpha, lambda
CASES = (
    (1, 2, 1, 1, 0, 1, 0.0, 0.5),
    (2, 3, 5, 3, 1, 1, 1.0, 0.5),
    (3, 63, 70, 3, 36, 3, 40.0, 10.0),
    (15, 64, 70, 50, 36, 1, 0.0, 0.5),
    (16, 65, 300, 65, 36, 3, 1.0, 0.5),
    # filler_num = I - 1 - n_targets: fake rows of 199 > 3 RK_IALS_CHUNK entries.  alpha = 40 makes wbar = 200, and the rounding of
    # a d-long dot times wbar (the "amplified" part of the budgets of h and grad) then passes 2^-10 of the stage's largest value
    # on some shapes (computed: 1.5e-3 at d = 15 x 64 items, 3.4e-3 at d = 127 x 63 items, 2.4e-3 on this long row), so (40, 10)
    # goes to d = 3, d = 31 and the defaults' shape, where the cap holds, and those three take the smaller alphas
    (17, 200, 70, 3, 196, 3, 1.0, 0.5),
    (31, 257, 300, 50, 36, 1, 40.0, 10.0),
    (32, 1100, 70, 3, 1, 1, 1.0, 0.5),
    (33, 200, 5, 1, 198, 1, 0.0, 0.5),              # filler_num = I - 1 - n_targets
    (64, 64, 300, 3, 0, 3, 0.0, 0.5),
    (65, 200, 70, 65, 36, 1, 1.0, 0.5),
    (127, 63, 70, 3, 36, 1, 0.0, 0.5),
    (128, 257, 70, 50, 1, 3, 1.0, 0.5),
    (16, 200, 300, 50, 36, 1, 40.0, 10.0),          # the defaults' shape in small
)
RATING = 5.0


def case_id(c):
    return f"d{c[0]}-I{c[1]}-U{c[2]}-A{c[3]}-F{c[4]}-t{c[5]}-a{c[6]:g}-l{c[7]:g}"


@functools.lru_cache(maxsize=None)
def case(c):
    """The data of one case: the real CSR (density 0.15, ratings 1..5; user 0 has rated everything but the first target when
    there are at least five users), the targets, the binarised fake rows and Yo (two float64 sweeps on the real data from a
    0.01 normal table, rounded to fp32)."""
    d, I, U, A, F, n_t, alpha, lam = c
    rng = np.random.default_rng(104729 * CASES.index(c) + 7)
    targets = np.sort(rng.permutation(I)[:n_t]).tolist()
    rows = []
    for u in range(U):
        if u == 0 and U >= 5:
            r = np.setdiff1d(np.arange(I), [targets[0]])
        else:
            r = np.where(rng.random(I) < 0.15)[0]
            if U < 5 or u == 1:
                r = np.setdiff1d(r, targets)            # every target keeps an eligible user
        rows.append(r)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    idx = np.concatenate(rows + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    val = rng.integers(1, 6, size=len(idx)).astype(np.float32)
    others = np.setdiff1d(np.arange(I), targets)
    cols = np.stack([np.sort(np.concatenate([targets, rng.choice(others, size=F, replace=False)])).astype(np.int64) for _ in range(A)])
    Y0 = 0.01 * rng.standard_normal((I, d))
    _, Yo = IR.fit64(ptr, idx, val, I, Y0, alpha, lam, 2)
    return {"d": d, "I": I, "U": U, "A": A, "F": F, "targets": targets, "alpha": alpha, "lam": lam, "ptr": ptr, "idx": idx, "val": val,
            "cols": cols, "Yo": Yo.astype(np.float32), "wbar": wbar32(alpha, RATING), "rng_seed": 104729 * CASES.index(c) + 11}


@functools.lru_cache(maxsize=None)
def chain(c):
    k = case(c)
    return chain64(k["ptr"], k["idx"], k["val"], k["I"], k["cols"], k["Yo"], k["targets"], k["alpha"], k["lam"], RATING)
