"""NumPy restatement of one LightGCN train step of the C-ABI handle (recad_amd/csrc/lightgcn.hip, rk_lightgcn_*; the walk of
lightgcn.py:82-169): the seeded graph / triplet / state inputs, the float64 walk of a step with the error budget of every
element, the separately rounded fp32 Adam, and an fp32 restatement of the step with planted faults (test_lightgcn_step_host.py
shows that the correct fp32 step stays inside the budgets and that every fault leaves them; test_lightgcn_step_gpu.py holds the
kernels to them).  No GPU, no torch.  The BPR stage, the SpMM row budget and the Adam budget are those of
tests/_sharded_ops_restate.py (R below); what is added here is how they chain.

A step is walked from the fp32 state it starts from, never from the reference's own earlier steps, so budgets do not compound.
Beside every float64 quantity the walk carries a budget b of what a correct fp32 implementation may be off by; u = 2^-24:
  * forward layer l, x_l = A x_{l-1}: b(x_l) = |A| b(x_{l-1}) + (nnz_r + 3) u |A| |x_{l-1}| -- per row nnz_r products (the row
    gather multiplies val[e] x[c] by FMA, the LDS kernel rounds dinv[c] x[c] and scales the row's sum by dinv[r] once: one more
    rounding) and nnz_r - 1 additions in any order, each against sum|term| (R.spmm_ex);
  * the running layer sum s_l = s_{l-1} + x_l rounds once per layer: + u |s_l|; light = s_L / (L + 1) is a product with the
    fp32 1 / (L + 1): the `sum_scale` product and the rounding of 1 / (L + 1) itself, 2 u |light|.  L = 0 copies E0: budget 0;
  * BPR: R.bpr_bounds (dot products, expf / log1pf, 1 / nb, the incidence sums in any order -- which covers the atomic adds'
    unknown order and the plan order alike) for exact light rows, plus what light's own budget does: x_b moves by at most
    dxl_b = sum_k b(lu) |ln - lp| + |lu| (b(ln) + b(lp)), which scales a term like rho_b does, and the term's vector factor
    moves by dx_b b(.); the loss takes mean(dxl_b) more (softplus' <= 1);
  * backward layer j, t_j = A t_{j-1} + add (add = gprop, the last layer gego): b(t_j) = |A| b(t_{j-1}) + b(add) +
    (nnz_r + 3) u (|A| |t_{j-1}| + |add|);
  * the counted regulariser of the LDS path (the last backward layer adds creg * cnt * E0 in closed form instead of scattering
    it): lambda / nb is two roundings (1 / nb, the product), times float(cnt), times E0, added to the row: 6 u |reg| + u |grad|;
  * Adam: R.adam_param_bound for p; m' = m + w1 (g - m) moves by w1 b(g) and rounds three times, v' = v b2 + w2 g g moves by
    w2 (2 |g| + b(g)) b(g) and rounds four times; w1 / w2 are fp32: 4 u (|m| + |g|) and 5 u (|v| + g^2).

The weights: the row gather multiplies by the fp32 val[] of rk_build_norm_adj, the LDS kernel by dinv[r] dinv[c] with
dinv = fl(1 / sqrt(deg)) (host/lds_plan_host.h); the two differ in the last bits, so each path is walked with its own."""
import numpy as np

from . import _sharded_ops_restate as R

U32 = R.U32
SENTINEL = R.SENTINEL
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
BATCH = 96
N_TRIP = 3 * BATCH - 19                    # three steps, the last one ragged with 77 triplets
RUN = (36, 34)                             # the dual-role item: positive of 36 triplets and negative of 34 others, a run of 70
USER_RUN = 17

# ---------------------------------------------------------------- inputs
# The hub item is rated by every user that rates anything.  The schedule cuts a row into 64-nonzero segments and a workgroup has
# four waves, so a row is "long" (pieces of several workgroups that meet in the scratch block) from 257 nonzeros on: a hub of
# 129 users (the 130-user graph) leaves scratch_words at 0, 260 users are what the long-row path needs.  N = 351 = 10 * 32 + 31.
N_USERS, N_ITEMS = 261, 90
ISO_USER, HUB_ITEM, ISO_ITEM, DUAL_ITEM, USER17 = 3, 0, 5, 7, 10
# interactions per user beside the hub: both sides of dim / 4 = 16, 25 and 64 (the packed and the segment path of spmm.h); the
# rows past 64 nonzeros are few, so that the schedule keeps 64-nonzero segments
DEGREES = (1, 4, 9, 14, 15, 16, 23, 24, 25, 30)
BIG_DEGREES = {20: 62, 21: 63, 22: 64, 23: 80}
# the marked-block list (L = 3) needs 2 (3 batch + row_blocks_extra) <= plain schedule blocks: users of 17..20 interactions take
# a wave each, four to a workgroup
N_USERS2, N_ITEMS2 = 2300, 600


def graph(which=1):
    """binary interactions as a user -> item CSR (item ids ascending per user) -> dict"""
    if which == 1:
        U, I = N_USERS, N_ITEMS
        rng = np.random.default_rng(11)
        pool = np.array([i for i in range(I) if i not in (HUB_ITEM, ISO_ITEM)])
        rows = []
        for u in range(U):
            if u == ISO_USER:
                rows.append(np.zeros(0, dtype=np.int32))
                continue
            k = BIG_DEGREES.get(u, DEGREES[u % len(DEGREES)])
            rows.append(np.sort(np.append(rng.choice(pool, k, replace=False), HUB_ITEM)).astype(np.int32))
    else:
        U, I = N_USERS2, N_ITEMS2
        rng = np.random.default_rng(12)
        pool = np.arange(1, I)
        rows = [np.sort(np.append(rng.choice(pool, 16 + u % 4, replace=False), 0)).astype(np.int32) for u in range(U)]
    r_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return {"U": U, "I": I, "N": U + I, "r_ptr": r_ptr, "r_idx": np.concatenate(rows).astype(np.int32)}


def adjacency(g):
    """(rowptr, col) of the symmetric bipartite adjacency in the order of rk_build_norm_adj: user rows, then item rows with users
    ascending"""
    U, I = g["U"], g["I"]
    users = np.repeat(np.arange(U), np.diff(g["r_ptr"]))
    items = g["r_idx"].astype(np.int64)
    order = np.lexsort((users, items))
    col = np.concatenate([U + items, users[order]]).astype(np.int32)
    deg = np.concatenate([np.diff(g["r_ptr"]), np.bincount(items, minlength=I)])
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), col


def host_val(rowptr, col):
    """the adjacency's fp32 values as a host computes them (the GPU tests read the device's own instead)"""
    deg = np.diff(rowptr).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0).astype(np.float32)
    rows = np.repeat(np.arange(len(deg)), np.diff(rowptr))
    return (dinv[rows] * dinv[col]).astype(np.float32)


class Operator:
    """the dense float64 matrix a path multiplies by: path "rg" val[] as given, "lds" dinv[r] dinv[c] of the plan builder"""

    def __init__(self, rowptr, col, val, path, n_users):
        n = len(rowptr) - 1
        self.U = n_users
        self.n, self.rowptr, self.col, self.path = n, np.asarray(rowptr), np.asarray(col), path
        self.nnz = np.diff(rowptr).astype(np.float64)[:, None]
        self.rows = np.repeat(np.arange(n), np.diff(rowptr))
        deg = np.diff(rowptr).astype(np.float64)
        self.dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0).astype(np.float32)
        self.val = np.asarray(val, dtype=np.float32)
        w = self.val.astype(np.float64) if path == "rg" else self.dinv[self.rows].astype(np.float64) * self.dinv[self.col].astype(np.float64)
        self.A = np.zeros((n, n))
        self.A[self.rows, self.col] = w

    def mul(self, x, bx, add=None, badd=None):
        """v = A x (+ add) and its budget"""
        v, mag, b = self.A @ x, self.A @ np.abs(x), self.A @ bx
        if add is not None:
            v, mag, b = v + add, mag + np.abs(add), b + badd
        return v, b + (self.nnz + 3) * U32 * mag


def triplets(g, seed=5):
    """(users, pos, neg) int64 of the epoch: N_TRIP triplets, item ids (not node rows).  Step 0: DUAL_ITEM RUN[0] times positive
    and RUN[1] times negative, USER17 USER_RUN times, ISO_ITEM as a negative, everything else from the lower halves of the users
    and items; step 1: the upper halves only, so its rows are disjoint from step 0's; step 2 (77 triplets): anything."""
    rng = np.random.default_rng(seed)
    U, I = g["U"], g["I"]
    lo_u = np.array([u for u in range(U // 2) if u not in (ISO_USER, USER17)])
    hi_u = np.arange(U // 2, U)
    lo_i = np.array([i for i in range(I // 2) if i not in (ISO_ITEM, DUAL_ITEM)])
    hi_i = np.arange(I // 2, I)
    u0 = rng.choice(lo_u, BATCH)
    p0, n0 = rng.choice(lo_i, BATCH), rng.choice(lo_i, BATCH)
    slots = rng.permutation(BATCH)
    p0[slots[:RUN[0]]] = DUAL_ITEM
    n0[slots[RUN[0]:RUN[0] + RUN[1]]] = DUAL_ITEM
    u0[slots[-USER_RUN:]] = USER17
    n0[slots[RUN[0] + RUN[1]]] = ISO_ITEM
    u1, p1, n1 = rng.choice(hi_u, BATCH), rng.choice(hi_i, BATCH), rng.choice(hi_i, BATCH)
    r = N_TRIP - 2 * BATCH
    all_u = np.array([u for u in range(U) if u != ISO_USER])
    u2, p2, n2 = rng.choice(all_u, r), rng.integers(0, I, r), rng.integers(0, I, r)
    users, pos, neg = (np.concatenate(a).astype(np.int64) for a in ((u0, u1, u2), (p0, p1, p2), (n0, n1, n2)))
    same = np.nonzero(pos == neg)[0]      # two random picks that met (the dual-role slots never do: lo_i excludes that item)
    neg[same] = np.where(same < BATCH, lo_i[(np.searchsorted(lo_i, neg[same]) + 1) % len(lo_i)],
                         np.where(same < 2 * BATCH, hi_i[(neg[same] - hi_i[0] + 1) % len(hi_i)], (neg[same] + 1) % I))
    assert not np.any(pos == neg)
    return users, pos, neg


def window(trip, step):
    """the triplets of a step and their count"""
    lo, hi = step * BATCH, min((step + 1) * BATCH, len(trip[0]))
    return tuple(a[lo:hi] for a in trip), hi - lo


def node_rows(g, win):
    u, p, n = win
    return u, g["U"] + p, g["U"] + n


def state(g, d, seed):
    """E0 ~ 0.1 N(0, 1) like the model's init, moments on the scale of this step's gradients (m ~ 1e-4, v ~ 1e-8) so that a
    gradient error shows in all three of p, m, v.  The dual-role item's own embedding is four times as large: its gradient row
    is made of the users' rows, so its budget does not grow with it, and one lambda / nb E0 too few (1e-6 |E0|) stands out of
    70 incidences' roundings at L = 0 too, where the terms are largest."""
    rng = np.random.default_rng(seed)
    N = g["N"]
    E0 = (0.1 * rng.standard_normal((N, d))).astype(np.float32)
    E0[g["U"] + DUAL_ITEM] *= 4
    return E0, (1e-4 * rng.standard_normal((N, d))).astype(np.float32), (1e-8 * (rng.random((N, d)) + 0.5)).astype(np.float32)


# (variant, dim, L, lambda, adam_t0).  Every variant at least once, every dim and every L on both paths where the path has it
# (L = 0 is the row gather's alone, L = 5 the two multi-phase launches of lds_sync), lambda = 0 and 0.5 once on each path, t0 = 0, 1, 7.
# "rg": row gather, "lds": the LDS-resident kernel; bits / blocks / cnt / sync name the descriptor options given.
CASES = (
    ("rg", 64, 0, 1e-4, 0), ("rg", 100, 1, 0.5, 1), ("rg", 256, 2, 1e-4, 7), ("rg", 64, 3, 1e-4, 1),
    ("rg_bits", 64, 2, 1e-4, 7), ("rg_bits", 256, 3, 1e-4, 0), ("rg_bits", 100, 2, 0.0, 1), ("rg_bits", 64, 1, 1e-4, 0),
    ("rg_bits_cnt", 64, 2, 1e-4, 7),
    ("rg_blocks", 64, 3, 1e-4, 1),
    ("lds_cnt", 64, 1, 1e-4, 0), ("lds_cnt", 100, 2, 1e-4, 1), ("lds_cnt", 256, 3, 1e-4, 7),
    ("lds", 64, 3, 0.5, 1), ("lds", 256, 1, 1e-4, 0), ("lds", 100, 2, 1e-4, 7),
    ("lds_cnt_sync", 64, 2, 1e-4, 0), ("lds_cnt_sync", 100, 5, 1e-4, 7), ("lds_cnt_sync", 256, 3, 0.0, 1),
)


def case_id(c):
    return f"{c[0]}-d{c[1]}-L{c[2]}-lam{c[3]:g}-t{c[4]}"


def path_of(variant):
    return "lds" if variant.startswith("lds") else "rg"


def counted(variant, ordered):
    """is the regulariser applied in closed form by the last backward launch (LDS path, cnt given, atomic scatter)"""
    return variant.startswith("lds_cnt") and not ordered


def graph_of(variant):
    return 2 if variant == "rg_blocks" else 1


# ---------------------------------------------------------------- the float64 walk
def propagate64(op, E0, L):
    """(light, budget)"""
    x = s = np.asarray(E0, dtype=np.float64)
    if L == 0:
        return s, np.zeros_like(s)
    bx = bs = np.zeros_like(s)
    for _ in range(L):
        x, bx = op.mul(x, bx)
        s = s + x
        bs = bs + bx + U32 * np.abs(s)
    light = s / (L + 1)
    return light, bs / (L + 1) + 2 * U32 * np.abs(light)


def step64(op, E0, L, lam, rows, nb, closed_reg):
    """one step's float64 walk from the fp32 table E0 -> dict: light / loss / grad with budgets b_*, n (incidence counts)"""
    ru, rp, rn = rows
    E = np.asarray(E0, dtype=np.float64)
    d = E.shape[1]
    light, bl = propagate64(op, E0, L)
    res = R.bpr(d, L, lam, light, E, ru, rp, rn, compact=False)
    b_gprop, b_gego, b_loss = R.bpr_bounds(res, d, lam, E, nb)
    lu, lp, ln = light[ru], light[rp], light[rn]
    dxl = (bl[ru] * np.abs(ln - lp) + np.abs(lu) * (bl[rn] + bl[rp])).sum(1)
    extra = np.zeros_like(E)
    dx = res["dx"][:, None]
    for (r, t), bvec in zip(res["terms"], (bl[rn] + bl[rp], bl[ru], bl[ru])):
        np.add.at(extra, r, np.abs(t) * dxl[:, None] + dx * bvec)
    b_gprop, b_gego, b_loss = b_gprop + extra, b_gego + extra, b_loss + float(dxl.mean())
    if L == 0:
        grad, bg = res["gego"], b_gego
    else:
        t, bt = res["gprop"], b_gprop
        for j in range(1, L + 1):
            last = j == L and not closed_reg
            t, bt = op.mul(t, bt, res["gego"] if last else res["gprop"], b_gego if last else b_gprop)
        if closed_reg:
            reg = res["n"][:, None] * (lam / nb) * E
            t = t + reg
            bt = bt + 6 * U32 * np.abs(reg) + U32 * np.abs(t)
        grad, bg = t, bt
    return {"light": light, "b_light": bl, "loss": res["loss"], "b_loss": b_loss, "grad": grad, "b_grad": bg, "n": res["n"],
            "gprop": res["gprop"], "b_gprop": b_gprop}


def adam64(p, g, bg, m, v, t):
    """(p', m', v') in float64 and their budgets given the gradient's"""
    p2, m2, v2 = R.adam_step(p, g, m, v, t, LR, B1, B2, EPS)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    w1, w2 = 1.0 - float(np.float32(B1)), 1.0 - float(np.float32(B2))
    bp = R.adam_param_bound(p, g, bg, m, v, t, LR, B1, B2, EPS)
    bm = w1 * bg + 4 * U32 * (np.abs(m) + np.abs(g))
    bv = w2 * (2 * np.abs(g) + bg) * bg + 5 * U32 * (np.abs(v) + g * g)
    return (p2, m2, v2), (bp, bm, bv)


def adam_coef32(t):
    """the step's two fp32 coefficients (common.h adam_coef: double arithmetic, rounded once)"""
    c = R.adam_coef(t, LR, B1, B2)
    return np.float32(c[0]), np.float32(c[1])


def adam32(p, g, m, v, coef, swap=False):
    """common.h adam_elem: every operation rounded to fp32 on its own, in its order -> (p', m', v').  swap: the planted fault"""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    step, bc2s = f(coef[0]), f(coef[1])
    w1, w2, b2, eps = f(1.0 - float(f(B1))), f(1.0 - float(f(B2))), f(B2), f(EPS)
    if swap:
        m, v = v, m
    m2 = m + w1 * (g - m)
    v2 = v * b2 + (w2 * g) * g
    with np.errstate(invalid="ignore"):
        den = np.sqrt(v2) / bc2s + eps
    p2 = p - step * (m2 / den)
    return (p2, v2, m2) if swap else (p2, m2, v2)


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an element whose budget is zero must be exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.all(np.isfinite(err)), "non-finite output"
    assert np.all(err[bound == 0] == 0), "an element with a zero budget is not exact"
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))


def ratio_mutant(got, ref, bound):
    """the same for a planted fault: an error on a zero-budget element counts as outside"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if not np.all(np.isfinite(err)) or np.any(err[bound == 0] != 0):
        return np.inf
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))


# ---------------------------------------------------------------- an fp32 step, right or with a planted fault
MUTANTS = ("drop_incidence", "reg_once_fewer", "ragged_invb", "inv_layers", "frontier_drop", "residue", "swap_mv")


def _sum32(n_rows, rows, terms, rng):
    """fp32 sums per row, the terms taken one after the other: in the order given, or shuffled"""
    out = np.zeros((n_rows, terms.shape[1]), dtype=np.float32)
    if rng is not None:
        k = rng.permutation(len(rows))
        rows, terms = rows[k], terms[k]
    np.add.at(out, rows, terms)
    return out


def _mul32(op, x, rng, add=None):
    f = np.float32
    if op.path == "rg":
        v = _sum32(op.n, op.rows, op.val[:, None] * x[op.col], rng)
    else:
        v = op.dinv[:, None] * _sum32(op.n, op.rows, op.dinv[op.col][:, None] * x[op.col], rng)
    return (v + add).astype(f) if add is not None else v.astype(f)


def step32(op, E0, m, v, L, lam, rows, nb, t, closed_reg, rng=None, mutant=None, residue=None):
    """the step in fp32 arithmetic.  rng: the summation orders (incidences, row entries) are shuffled (the atomic scatter);
    None: plan order.  Returns light, loss, grad and the Adam'd (p, m, v)."""
    f = np.float32
    ru, rp, rn = rows
    N, d = E0.shape
    inv_layers = f(1.0) / f(L if (mutant == "inv_layers" and L > 0) else L + 1)
    x = s = E0
    for _ in range(L):
        x = _mul32(op, x, rng)
        s = s + x
    light = (s * inv_layers).astype(f) if L else E0
    invb = f(1.0) / f(BATCH if mutant == "ragged_invb" else nb)
    lu, lp, ln = light[ru], light[rp], light[rn]
    xx = (lu * ln).sum(1, dtype=f) - (lu * lp).sum(1, dtype=f)
    with np.errstate(over="ignore"):
        sp = np.where(xx > 20, xx, np.log1p(np.exp(xx, dtype=f), dtype=f))
        dx = (np.where(xx > 20, f(1.0), f(1.0) / (f(1.0) + np.exp(-xx, dtype=f))) * invb * (f(1.0) / f(L + 1))).astype(f)
    reg = ((E0[ru] ** 2).sum(dtype=f) + (E0[rp] ** 2).sum(dtype=f) + (E0[rn] ** 2).sum(dtype=f))
    loss = float(sp.sum(dtype=f) * invb + f(lam) * (f(0.5) * reg * invb))
    idx = np.stack([ru, rp, rn], axis=1).reshape(-1)                                   # (b, role) order: the plan's order per row
    terms = np.stack([dx[:, None] * (ln - lp), -dx[:, None] * lu, dx[:, None] * lu], axis=1).reshape(-1, d).astype(f)
    keep = np.ones(len(idx), dtype=bool)
    dual = op.U + DUAL_ITEM
    if mutant == "drop_incidence":
        keep[np.nonzero(idx == dual)[0][40]] = False
    creg = f(lam) * invb
    cnt = np.bincount(idx[keep], minlength=N)
    if mutant == "reg_once_fewer":
        cnt[dual] -= 1
    gprop = _sum32(N, idx[keep], terms[keep], rng)
    if residue is not None:
        gprop = (gprop + residue).astype(f)
    if closed_reg or mutant == "reg_once_fewer":
        gego = (gprop + (creg * cnt.astype(f))[:, None] * E0).astype(f)
    else:
        gego = _sum32(N, idx[keep], (terms[keep] + creg * E0[idx[keep]]).astype(f), rng)
        if residue is not None:
            gego = (gego + residue).astype(f)
    if L == 0:
        grad = gego
    else:
        tcur = gprop
        for j in range(1, L + 1):
            last = j == L and not closed_reg
            src = tcur
            if mutant == "frontier_drop" and j == 1:
                src = tcur.copy()
                src[ru[0]] = 0
            tcur = _mul32(op, src, rng, gego if last else gprop)
        grad = (tcur + (creg * cnt.astype(f))[:, None] * E0).astype(f) if closed_reg else tcur
    return {"light": light, "loss": loss, "grad": grad, "gprop": gprop, "adam": adam32(E0, grad, m, v, adam_coef32(t), swap=mutant == "swap_mv")}
