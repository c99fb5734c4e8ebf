"""NumPy float64 restatement of the op-level C ABI the row-sharded and 2-D trainers build a step from (include/recad_hip.h:
rk_bpr_rows, rk_bpr_rows_ordered, rk_spmm_csr_ex, rk_adam_coef_advance, rk_rows_gather_masked / _zero / _mark_bits), the error
budgets of a correct fp32 implementation of each, and the seeded inputs the host and the GPU tests share
(test_sharded_ops_host.py shows that a correct fp32 implementation stays inside the budgets, test_sharded_ops_gpu.py holds the
kernels to them).  No GPU, no torch.

Budgets.  u = 2^-24 is the unit roundoff of fp32.  Nothing below is tuned: every factor counts roundings.
  * a dot product of d terms summed in ANY order, each product rounded: error <= (d + 8) u sum|a_k b_k| (d - 1 additions and one
    product per term, the rest is slack for the lane-group / wave combines and the final subtraction);
  * x = <lu, ln> - <lu, lp> therefore carries dx_b = (d + 8) u S_b, S_b = sum_k |lu_k| (|lp_k| + |ln_k|);
  * sigma(x) / nb / (L + 1): d ln sigma / dx <= 1 turns the absolute error of x into a relative one of sigma, and expf, 1 + e, the
    division, 1 / nb, 1 / (L + 1) and the two products add 8 u: rho_b = dx_b + 8 u;
  * a gradient element is a sum of n_r incidences in some order: every term carries rho_b of its triplet, its own two roundings,
    and the n_r - 1 additions each round a partial sum that is at most A = sum|term|: W + (n_r + 4) u A;
  * gego adds (lam / nb) emb per incidence: n_r more terms of that size under the same (n_r + 4) u;
  * the loss: softplus' = sigma <= 1 passes dx_b through, and the sum of positive terms (ceil(nb / 256) per workgroup in the
    atomic form, d squares per row, the group / wave / workgroup combines) is relative: (ceil(nb / 256) + d + 32) u loss.
  * SpMM row r: nnz_r products and additions plus the addend: (nnz_r + 3) u (sum|val x| + |add|); the running sum adds one
    addition and one product: 2 u (|sum_in| + |v|) |sum_scale|."""
import math

import numpy as np

U32 = 2.0 ** -24
HUBS = (1, 15, 16, 17, 63, 64, 65, 128, 129, 200)      # run lengths around the 16-incidence rounds and the 64-incidence chunks
DUAL = (33, 34)                                         # one item: positive of 33 triplets AND negative of 34 others (a run of 67)
SENTINEL = 7.0


# ---------------------------------------------------------------- BPR
def plan_keys(ru, rp, rn):
    """sorted uint64 keys (row << 20) | (3 b + role) of a batch (rk_bpr_rows_ordered)"""
    rows = np.stack([ru, rp, rn], axis=1).astype(np.uint64)                          # [nb, 3]
    inc = (3 * np.arange(len(ru), dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :])
    return np.sort(((rows << np.uint64(20)) | inc).reshape(-1))


def _light_rows(light, ru, rp, rn, compact):
    nb = len(ru)
    light = np.asarray(light, dtype=np.float64)
    if compact:
        return light[:nb], light[nb:2 * nb], light[2 * nb:3 * nb]
    return light[ru], light[rp], light[rn]


def bpr(dim, L, lam, light, emb, ru, rp, rn, compact=True):
    """bpr_kernel in float64.  light: the compact [3 nb, d] block (rows b, nb + b, 2 nb + b of triplet b), or with compact = False a
    table indexed by the rows; emb [N, d].  Returns a dict: gprop / gego [N, d] (the contributions, zero on untouched rows), loss,
    x / dx / S / rho per triplet, n [N] incidence counts, A / W [N, d] (module docstring)."""
    ru, rp, rn = (np.asarray(a, dtype=np.int64) for a in (ru, rp, rn))
    emb = np.asarray(emb, dtype=np.float64)
    nb, (N, d) = len(ru), emb.shape
    assert d == dim
    lu, lp, ln = _light_rows(light, ru, rp, rn, compact)
    x = (lu * ln).sum(1) - (lu * lp).sum(1)
    sig = np.exp(-np.logaddexp(0.0, -x))
    dx = sig / nb / (L + 1)
    terms = ((ru, dx[:, None] * (ln - lp)), (rp, -dx[:, None] * lu), (rn, dx[:, None] * lu))
    S = (np.abs(lu) * (np.abs(lp) + np.abs(ln))).sum(1)
    rho = (d + 8) * U32 * S + 8 * U32
    gprop, A, W = np.zeros((N, d)), np.zeros((N, d)), np.zeros((N, d))
    n = np.zeros(N, dtype=np.int64)
    for rows, t in terms:
        np.add.at(gprop, rows, t)
        np.add.at(A, rows, np.abs(t))
        np.add.at(W, rows, np.abs(t) * rho[:, None])
        np.add.at(n, rows, 1)
    gego = gprop + n[:, None] * (lam / nb) * emb
    reg = (emb[ru] ** 2).sum() + (emb[rp] ** 2).sum() + (emb[rn] ** 2).sum()
    loss = np.logaddexp(0.0, x).mean() + lam / 2 * reg / nb
    return {"gprop": gprop, "gego": gego, "loss": float(loss), "x": x, "dx": dx, "S": S, "rho": rho, "n": n, "A": A, "W": W,
            "terms": terms}


def bpr_bounds(res, dim, lam, emb, nb):
    """(bound_gprop [N, d], bound_gego [N, d], bound_loss) of a correct fp32 implementation (module docstring)"""
    n = res["n"][:, None].astype(np.float64)
    b_gprop = res["W"] + (n + 4) * U32 * res["A"]
    b_gego = b_gprop + (n + 4) * U32 * n * np.abs(lam / nb * np.asarray(emb, dtype=np.float64))
    dx_abs = (dim + 8) * U32 * res["S"]
    b_loss = dx_abs.mean() + (math.ceil(nb / 256) + dim + 32) * U32 * res["loss"]
    return b_gprop, b_gego, float(b_loss)


def bpr_case(nb, d, seed):
    """The BPR inputs of the tests: gathered node space N = 3 nb + 50, users in the lower half, items in the upper; light rows
    ~ N(0, 1) / sqrt(d) per NODE (light_tab [N, d]; `light` is its compact [3 nb, d] gather), emb ~ 0.1 N(0, 1); from 5 triplets on:
    triplets 0 and 1 on nodes of their own with rows scaled x 12 and x = +40 / -40 (the softplus / sigma switches), triplet 2 with
    rp == rn; one node per entry of HUBS with exactly that many incidences in one role (roles in turn; an entry that no longer fits
    the batch is left out), one item DUAL[0] times positive and DUAL[1] times negative; the leftover slots random over the other
    nodes, so run heads fall at arbitrary positions of the plan."""
    rng = np.random.default_rng(seed)
    N = 3 * nb + 50
    half = N // 2
    free_u, free_i = list(rng.permutation(half)), list(half + rng.permutation(N - half))
    rows = np.full((3, nb), -1, dtype=np.int64)
    slots = [list(rng.permutation(np.arange(3 if nb >= 5 else 0, nb))) for _ in range(3)]
    special = nb >= 5
    if special:
        for b in (0, 1):
            rows[:, b] = free_u.pop(), free_i.pop(), free_i.pop()
        rows[0, 2] = free_u.pop()
        rows[1, 2] = rows[2, 2] = free_i.pop()
    hubs = []
    for k, count in enumerate(HUBS):
        role = k % 3
        if count > len(slots[role]):
            continue
        node = free_u.pop() if role == 0 else free_i.pop()
        for _ in range(count):
            rows[role, slots[role].pop()] = node
        hubs.append((int(node), role, count))
    if DUAL[0] <= len(slots[1]) and DUAL[1] <= len(slots[2]):
        node = free_i.pop()
        taken = [slots[1].pop() for _ in range(DUAL[0])]
        rest = [s for s in slots[2] if s not in taken][:DUAL[1]]
        if len(rest) == DUAL[1]:
            rows[1, taken], rows[2, rest] = node, node
            slots[2] = [s for s in slots[2] if s not in rest]
            hubs.append((int(node), 1, DUAL[0]))
            hubs.append((int(node), 2, DUAL[1]))
        else:
            slots[1] += taken
            free_i.append(node)
    # leftover slots: random over a pool of the remaining nodes about as large as the batch (some repeats, most runs short)
    pool_u, pool_i = np.array(free_u[:max(1, min(len(free_u), nb))]), np.array(free_i[:max(2, min(len(free_i), nb))])
    for role, pool in ((0, pool_u), (1, pool_i), (2, pool_i)):
        todo = np.nonzero(rows[role] < 0)[0]
        rows[role, todo] = pool[rng.integers(0, len(pool), size=len(todo))]
    for b in np.nonzero(rows[1] == rows[2])[0]:       # two random picks that met (hub slots never do): the one rp == rn triplet is b = 2
        if not (special and b == 2):
            rows[2, b] = pool_i[(int(np.nonzero(pool_i == rows[1, b])[0][0]) + 1) % len(pool_i)]
    ru, rp, rn = rows
    light_tab = (rng.standard_normal((N, d)) / np.sqrt(d)).astype(np.float32)
    emb = (0.1 * rng.standard_normal((N, d))).astype(np.float32)
    if special:
        for b, target in ((0, 40.0), (1, -40.0)):
            u_, p_, n_ = rows[:, b]
            light_tab[u_] *= 12
            light_tab[p_] *= 12
            lu = light_tab[u_].astype(np.float64)
            light_tab[n_] = (light_tab[p_].astype(np.float64) + target / (lu * lu).sum() * lu).astype(np.float32)
    light = np.ascontiguousarray(np.concatenate([light_tab[ru], light_tab[rp], light_tab[rn]]))
    touched = np.zeros(N, dtype=bool)
    touched[rows.reshape(-1)] = True
    return {"nb": nb, "d": d, "N": N, "ru": ru.copy(), "rp": rp.copy(), "rn": rn.copy(), "light": light, "light_tab": light_tab, "emb": emb,
            "touched": touched, "hubs": hubs, "keys": plan_keys(ru, rp, rn)}


# (nb, d, L, lam): every batch size (1400: 4200 incidences, the second trip of the plan loop) at every width, with the workload's
# L = 3 / lambda = 1e-4 and with L = 0 / lambda = 0.5 (the reg term as large as the BPR term); lambda = 0 at the 5-triplet batch
BPR_DIMS = (64, 128, 256, 7, 50, 100, 130)
BPR_NB = (1, 5, 1061, 1400)
BPR_CASES = tuple((nb, d, L, lam) for nb in BPR_NB for d in BPR_DIMS for L, lam in ((3, 1e-4), (0, 0.5))) + tuple((5, d, 3, 0.0) for d in BPR_DIMS)
BPR_CASES_ATOMIC = BPR_CASES + tuple((nb, 300, L, lam) for nb in BPR_NB for L, lam in ((3, 1e-4), (0, 0.5))) + ((5, 300, 3, 0.0),)


def pad_keys(rows3, B):
    """the ragged-step plan of recad_amd/sharded.py _epoch_plan: [3, nb] gathered rows of a step of nb < B triplets in a batch-B plan,
    the tail padded with keys that sort behind everything -> sorted int64 [3 B]"""
    nb = rows3.shape[1]
    keys = (rows3.astype(np.int64) << 20) | (3 * np.arange(nb, dtype=np.int64)[None, :] + np.arange(3, dtype=np.int64)[:, None])
    padded = np.full((3, B), np.iinfo(np.int64).max, dtype=np.int64)
    padded[:, :nb] = keys
    return np.sort(padded.reshape(-1))


# ---------------------------------------------------------------- SpMM
def spmm_ex(csr, x, add=None, sum_in=None, sum_scale=1.0):
    """v = A x (+ add), sum_out = (sum_in + v) * sum_scale in float64, with the per-element budgets -> (v, bound_v, sum_out, bound_sum)
    (the last two None without sum_in)"""
    rowptr, col, val = csr
    x = np.asarray(x, dtype=np.float64)
    n, d = len(rowptr) - 1, x.shape[1]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    prod = np.asarray(val, dtype=np.float64)[:, None] * x[col]
    v, mag = np.zeros((n, d)), np.zeros((n, d))
    np.add.at(v, rows, prod)
    np.add.at(mag, rows, np.abs(prod))
    if add is not None:
        add = np.asarray(add, dtype=np.float64)
        v, mag = v + add, mag + np.abs(add)
    bound_v = (np.diff(rowptr)[:, None] + 3) * U32 * mag
    if sum_in is None:
        return v, bound_v, None, None
    sum_in, sc = np.asarray(sum_in, dtype=np.float64), float(np.float32(sum_scale))
    return v, bound_v, (sum_in + v) * sc, bound_v * abs(sc) + 2 * U32 * (np.abs(sum_in) + np.abs(v)) * abs(sc)


def spmm_slab(n, rect, seed, avg=12):
    """(csr, x_rows): ~n rows, two empty ones, Poisson(avg) rows on both sides of dim / 4 nonzeros, two medium rows, and row 5 with
    every column (the long row of the schedule); rect: x has 2 n rows"""
    from ._csr_rand import _rand_csr
    rng = np.random.default_rng(seed)
    x_rows = 2 * n if rect else n
    return _rand_csr(rng, n, avg, long_rows=[(5, x_rows), (77, 100), (200, 40), (9, 0), (10, 0)], n_cols=x_rows), x_rows


SPMM_DIMS = (32, 64, 128, 256, 48, 100)
SPMM_N = 600
# (add, y, running sum, zeroing): one field at a time, then all together
SPMM_FIELDS = {"y": (0, 1, 0, 0), "add": (1, 1, 0, 0), "sum": (0, 0, 1, 0), "zero": (0, 1, 0, 1), "all": (1, 1, 1, 1)}


def spmm_operands(n, x_rows, d, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"x": f(x_rows, d), "add": f(n, d), "sum_in": f(n, d), "sum_scale": float(np.float32(1.0 / 3.0))}


# ---------------------------------------------------------------- Adam
def adam_coef(t, lr, b1, b2):
    """{lr / (1 - b1^t), sqrt(1 - b2^t)} in float64 from the fp32 hyper-parameters the entry points take"""
    lr, b1, b2 = (float(np.float32(a)) for a in (lr, b1, b2))
    return lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


def adam_step(p, g, m, v, t, lr, b1, b2, eps):
    """torch.optim.Adam step t in float64 -> (p, m, v)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1f, b2f, epsf = (float(np.float32(a)) for a in (b1, b2, eps))
    step, bc2s = adam_coef(t, lr, b1, b2)
    m2 = m + (1.0 - b1f) * (g - m)
    v2 = v * b2f + (1.0 - b2f) * g * g
    return p - step * (m2 / (np.sqrt(v2) / bc2s + epsf)), m2, v2


def adam_param_bound(p, g, bound_g, m, v, t, lr, b1, b2, eps):
    """budget of the updated parameter when the gradient is only known to bound_g: the mean value theorem over [g - bound_g,
    g + bound_g] (|dp/dg| <= step (w1 / den + |m'| w2 |g| / (sqrt(v') bc2s den^2)) at the interval's worst ends) plus the roundings
    of the update itself: 16 u on the step (m' three, v' three and its root, the two divisions, eps, the product, w1 / w2 / the
    coefficients as fp32) and u on the final subtraction's result, |p'| <= |p| + |step|"""
    p, g, m, v, bg = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v, bound_g))
    b1f, b2f, epsf = (float(np.float32(a)) for a in (b1, b2, eps))
    step, bc2s = adam_coef(t, lr, b1, b2)
    w1, w2 = 1.0 - b1f, 1.0 - b2f
    g_hi, g_lo = np.abs(g) + bg, np.maximum(np.abs(g) - bg, 0.0)
    m_hi = np.abs(m) * b1f + w1 * g_hi
    v_lo = v * b2f + w2 * g_lo * g_lo
    den_lo = np.sqrt(v_lo) / bc2s + epsf
    slope = step * (w1 / den_lo + m_hi * w2 * g_hi / (np.maximum(np.sqrt(v_lo), 1e-300) * bc2s * den_lo ** 2))
    upd = step * m_hi / den_lo
    return slope * bg + 16 * U32 * upd + U32 * (np.abs(p) + upd)


# ---------------------------------------------------------------- index kernels
def gather_masked(src, idx, mask):
    """out[i] = mask[i] * src[idx[i]] in fp32, a zero mask entry giving +0.0 whatever the row holds"""
    rows = np.asarray(src, dtype=np.float32)[idx]
    if mask is None:
        return rows.copy()
    m = np.asarray(mask, dtype=np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(m != 0, rows * m, np.float32(0.0)).astype(np.float32)


def zero_rows(a, idx):
    out = np.array(a, copy=True)
    out[idx] = 0
    return out


def mark_bits(bits, idx, set_):
    """bits |= the idx bits (set_), or the words holding an idx bit = 0"""
    out = np.array(bits, dtype=np.uint32, copy=True)
    idx = np.asarray(idx, dtype=np.int64)
    if set_:
        np.bitwise_or.at(out, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    else:
        out[idx >> 5] = 0
    return out
