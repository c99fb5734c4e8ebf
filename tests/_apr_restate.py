"""NumPy restatement of the APR victim's train step (include/recad_hip.h, "APR victim"; csrc/apr.hip), stage by stage in float64,
the fp32 walk of steps 2 and 5 in key order (what the kernels must reproduce to the bit), the error budgets of a correct fp32
implementation of every other stage, and the seeded cases the host and the GPU tests share.  No GPU, no torch.

Every stage is restated from the inputs it is GIVEN, so a test feeds it what the implementation under test produced for the
stage before (check_chain): an error is charged to the stage that made it.

Budgets.  u = 2^-24.  Nothing below is tuned: every factor counts roundings.  Taken as they stand from
tests/_sharded_ops_restate.py, where rk_bpr_rows holds them:
  * a dot of d terms in any order: (d + 8) u sum|a_k b_k|; so x carries dx_b = (d + 8) u S_b, S_b = sum_k |p_k| (|q_ik| + |q_jk|);
  * the coefficient c_b = sigma(x_b) / B, relative: rho_b = dx_b + 8 u;
  * a loss (L, L', and R, whose d squares per row are summed like a dot): mean_b dx_b + (ceil(B / 256) + d + 32) u loss.
New here:
  * n_r from a given Gamma: d squares (one rounding each) and d - 1 additions in any order put at most d u, relatively, on the sum
    of squares (all terms are >= 0: no cancellation); the square root halves that and rounds once; one more u for the second-order
    terms: relative (d / 2 + 2) u;
  * Delta from a given Gamma: eps as an fp32, the division eps / max(n_r, 1e-12) and the product Gamma * s are three more roundings:
    relative (d / 2 + 5) u; a row whose Gamma is all zero is exactly zero (0 * s, s finite);
  * p + Delta: one rounding per element, |fl(p + D) - (p + D)| <= u |p + D|;
  * x' from the given Delta: the dot budget on the moved rows, (d + 8) u S', plus what the roundings of the moved rows themselves do
    to the two dots: u |p'_k| |q'_jk - q'_ik| for p' and u |p'_k| (|q'_ik| + |q'_jk|) for the q', at most 2 u S' together;
  * c' and L' as c and L, from dx' = (d + 10) u S'.
Steps 2 and 5 are exact on the device (compared with walk_gamma32 / walk_grad32 bit for bit).  For an fp32 implementation in ANOTHER
order, and for the planted defects, they carry budgets too.  A row of n incidences with magnitudes A = sum over its incidences of
|c| (|q_j| + |q_i|) or |c| |p| (plus adv_reg |c'| times the same of the moved rows, plus (lambda / B) |self| in step 5):
  * Gamma from a given c: two roundings per term and n - 1 additions of partial sums that are at most A: (n + 4) u A;
  * the gradient from given c, c', Delta: three additions per incidence and at most five roundings per term (q + Delta, the
    difference, c' *, adv_reg *, lambda / B): (3 n + 8) u A."""
import math

import numpy as np

from . import _sharded_ops_restate as S

U32 = S.U32
HUBS, DUAL = S.HUBS, S.DUAL
N_USERS, N_ITEMS = 40, 70
LAM, EPS, ADV_REG = 0.01, 0.5, 0.5      # adv_reg != 1, so that a factor on the wrong term shows
SENTINEL = 7.0
TINY_NORM = 1e-12


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sigmoid(x):
    return np.exp(-np.logaddexp(0.0, -x))


# ---------------------------------------------------------------- the plan
def plan(u, i, j, U):
    """sorted keys (row << 20 | 3 b + role) of ONE step and what the kernels derive from them: `starts` (n_slots + 1 sorted
    positions, the run table), `rows` (the row of each slot), `slot_of` [3 nb], `krow` / `kinc` per sorted position"""
    u, i, j = (np.asarray(a, dtype=np.int64) for a in (u, i, j))
    nb = len(u)
    rows3 = np.stack([u, U + i, U + j], axis=1)
    inc = 3 * np.arange(nb, dtype=np.int64)[:, None] + np.arange(3, dtype=np.int64)[None, :]
    keys = np.sort(((rows3.astype(np.uint64) << np.uint64(20)) | inc.astype(np.uint64)).reshape(-1))
    krow, kinc = (keys >> np.uint64(20)).astype(np.int64), (keys & np.uint64((1 << 20) - 1)).astype(np.int64)
    head = np.r_[True, krow[1:] != krow[:-1]]
    starts = np.r_[np.nonzero(head)[0], 3 * nb]
    slot_of = np.empty(3 * nb, dtype=np.int64)
    slot_of[kinc] = np.cumsum(head) - 1
    return {"keys": keys, "krow": krow, "kinc": kinc, "starts": starts, "rows": krow[starts[:-1]], "slot_of": slot_of,
            "n": np.diff(starts), "nb": nb}


# ---------------------------------------------------------------- float64 stages
def coef64(tab, u, i, j, U, lam, delta_rows=None, nb=None):
    """steps 1 / 4: x, c, the loss, R, and S per triplet.  delta_rows: ([nb, d], [nb, d], [nb, d]) moves the rows first."""
    tab = np.asarray(tab, dtype=np.float64)
    p, qi, qj = tab[u], tab[U + i], tab[U + j]
    if delta_rows is not None:
        p, qi, qj = (a + np.asarray(b, dtype=np.float64) for a, b in zip((p, qi, qj), delta_rows))
    nb = len(u) if nb is None else nb
    x = (p * qj).sum(1) - (p * qi).sum(1)
    Sx = (np.abs(p) * (np.abs(qi) + np.abs(qj))).sum(1)
    return {"x": x, "c": sigmoid(x) / nb, "L": float(np.logaddexp(0.0, x).sum() / nb), "S": Sx,
            "R": float(lam / (2 * nb) * ((p * p).sum() + (qi * qi).sum() + (qj * qj).sum()))}


def _terms(tab, u, i, j, U, c, delta_rows=None):
    """per incidence [nb, 3, d]: the term of step 2 and its magnitude |c| (|q_j| + |q_i|) / |c| |p|"""
    tab = np.asarray(tab, dtype=np.float64)
    p, qi, qj = tab[u], tab[U + i], tab[U + j]
    if delta_rows is not None:
        p, qi, qj = (a + np.asarray(b, dtype=np.float64) for a, b in zip((p, qi, qj), delta_rows))
    c = np.asarray(c, dtype=np.float64)[:, None]
    T = np.stack([c * (qj - qi), -c * p, c * p], axis=1)
    M = np.stack([np.abs(c) * (np.abs(qj) + np.abs(qi)), np.abs(c) * np.abs(p), np.abs(c) * np.abs(p)], axis=1)
    return T, M


def _by_slot(pl, T):
    out = np.zeros((len(pl["rows"]), T.shape[2]))
    np.add.at(out, pl["slot_of"], T.reshape(-1, T.shape[2]))
    return out


def gamma64(tab, u, i, j, U, c, pl):
    """step 2 from a given c -> (Gamma [n_slots, d], A [n_slots, d])"""
    T, M = _terms(tab, u, i, j, U, c)
    return _by_slot(pl, T), _by_slot(pl, M)


def delta64(gamma, eps):
    """step 3 from a given Gamma -> (n [n_slots], Delta)"""
    g = np.asarray(gamma, dtype=np.float64)
    n = np.sqrt((g * g).sum(1))
    return n, g * (float(np.float32(eps)) / np.maximum(n, TINY_NORM))[:, None]


def delta_rows_of(delta, pl):
    so = pl["slot_of"].reshape(-1, 3)
    return delta[so[:, 0]], delta[so[:, 1]], delta[so[:, 2]]


def grad64(tab, u, i, j, U, c, c_adv, delta, pl, lam, adv_reg, nb=None):
    """step 5 from given c, c', Delta -> (dense gradient [N, d], A [N, d])"""
    tab = np.asarray(tab, dtype=np.float64)
    nb = len(u) if nb is None else nb
    T, M = _terms(tab, u, i, j, U, c)
    if adv_reg != 0:
        Ta, Ma = _terms(tab, u, i, j, U, c_adv, delta_rows_of(np.asarray(delta, dtype=np.float64), pl))
        T, M = T + adv_reg * Ta, M + adv_reg * Ma
    selfs = np.stack([tab[u], tab[U + i], tab[U + j]], axis=1)
    T, M = T + lam / nb * selfs, M + lam / nb * np.abs(selfs)
    g, A = np.zeros_like(tab), np.zeros_like(tab)
    g[pl["rows"]], A[pl["rows"]] = _by_slot(pl, T), _by_slot(pl, M)
    return g, A


def step64(tab, u, i, j, U, lam, eps, adv_reg, nb=None, defect=None):
    """the whole step in float64 -> every stage.  nb: the 1 / B to use (a planted defect); defect: one of DEFECTS."""
    pl = plan(u, i, j, U)
    tab = np.asarray(tab, dtype=np.float64)
    out = {"plan": pl, "slot_of": pl["slot_of"]}
    one = coef64(tab, u, i, j, U, lam, nb=nb)
    out.update({k: one[k] for k in ("x", "c", "L", "R")})
    if adv_reg == 0:
        out["grad"], _ = grad64(tab, u, i, j, U, one["c"], None, None, pl, lam, 0.0, nb=nb)
        out["L_adv"] = 0.0
        return out
    G, _ = gamma64(tab, u, i, j, U, one["c"], pl)
    if defect == "gamma_with_lambda":
        G = G + lam / len(u) * pl["n"][:, None] * tab[pl["rows"]]
    if defect == "dual_two_rows":       # the item that is positive here and negative there: each role sums on its own and only
        T, _ = _terms(tab, u, i, j, U, one["c"])        # the positive half is kept
        for s, r in enumerate(pl["rows"]):
            roles = pl["kinc"][pl["starts"][s]:pl["starts"][s + 1]] % 3
            if r >= U and len(set(roles)) == 2:
                G[s] = sum(T[inc // 3, 1] for inc in pl["kinc"][pl["starts"][s]:pl["starts"][s + 1]] if inc % 3 == 1)
    n, D = delta64(G, eps)
    if defect == "one_norm":
        n = np.full_like(n, math.sqrt((G * G).sum()))
        D = G * (eps / max(n[0], TINY_NORM))
    if defect == "minus_delta":
        D = -D
    if defect == "no_norm":
        D = eps * G
    rows = list(delta_rows_of(D, pl))
    if defect == "no_delta_on_negative":
        rows[2] = np.zeros_like(rows[2])
    two = coef64(tab, u, i, j, U, lam, delta_rows=rows, nb=nb)
    g, _ = grad64(tab, u, i, j, U, one["c"], two["c"], D, pl, lam, adv_reg, nb=nb)
    if defect == "adv_reg_on_data":
        g0, _ = grad64(tab, u, i, j, U, one["c"], None, None, pl, 0.0, 0.0, nb=nb)
        g = g - (1 - adv_reg) * g0
    out.update({"gamma": G, "norm": n, "delta": D, "x_adv": two["x"], "c_adv": two["c"], "L_adv": two["L"], "grad": g})
    return out


DEFECTS = ("one_norm", "gamma_with_lambda", "no_delta_on_negative", "minus_delta", "no_norm", "adv_reg_on_data", "dual_two_rows")


# ---------------------------------------------------------------- fp32
def walk_gamma32(tab, u, i, j, U, c, pl, reverse=False):
    """step 2 as the kernel walks it: per slot from +0.0, per incidence in key order acc = fl(acc + fl(cs * part)), part =
    fl(q_j - q_i) for the user and p_u for an item, cs = c, -c (positive) or c (negative).  Bits.  reverse: the incidences from
    the last to the first, ANOTHER order (not the kernel's), for the budgets."""
    tab, c = np.ascontiguousarray(tab, dtype=np.float32), np.ascontiguousarray(c, dtype=np.float32)
    out = np.zeros((len(pl["rows"]), tab.shape[1]), dtype=np.float32)
    for s in range(len(pl["rows"])):
        acc = np.zeros(tab.shape[1], dtype=np.float32)
        for inc in pl["kinc"][pl["starts"][s]:pl["starts"][s + 1]][::-1 if reverse else 1]:
            b, role = divmod(int(inc), 3)
            if role == 0:
                acc = acc + c[b] * (tab[U + j[b]] - tab[U + i[b]])
            else:
                acc = acc + (-c[b] if role == 1 else c[b]) * tab[u[b]]
        out[s] = acc
    return out


def walk_grad32(tab, u, i, j, U, c, c_adv, delta, pl, lam, adv_reg, nb=None, reverse=False):
    """step 5 as the kernel walks it: per incidence (a) the term of step 2, (b) fl(adv_reg * fl(cs' * part')) from the moved rows
    fl(q + Delta) -- left out when adv_reg == 0 --, (c) fl(fl(lambda / (float) B) * self), each added on its own.  Dense bits."""
    tab, c = np.ascontiguousarray(tab, dtype=np.float32), np.ascontiguousarray(c, dtype=np.float32)
    nb = len(u) if nb is None else nb
    lam_b, adv = np.float32(lam) / np.float32(nb), np.float32(adv_reg)
    so = pl["slot_of"]
    out = np.zeros_like(tab)
    if adv_reg != 0:
        c_adv, delta = np.ascontiguousarray(c_adv, dtype=np.float32), np.ascontiguousarray(delta, dtype=np.float32)
    for s, row in enumerate(pl["rows"]):
        acc, self_ = np.zeros(tab.shape[1], dtype=np.float32), tab[row]
        for inc in pl["kinc"][pl["starts"][s]:pl["starts"][s + 1]][::-1 if reverse else 1]:
            b, role = divmod(int(inc), 3)
            if role == 0:
                v0, v1 = tab[U + i[b]], tab[U + j[b]]
                acc = acc + c[b] * (v1 - v0)
                if adv_reg != 0:
                    acc = acc + adv * (c_adv[b] * ((v1 + delta[so[3 * b + 2]]) - (v0 + delta[so[3 * b + 1]])))
            else:
                sign = np.float32(-1.0 if role == 1 else 1.0)
                v0 = tab[u[b]]
                acc = acc + (sign * c[b]) * v0
                if adv_reg != 0:
                    acc = acc + adv * ((sign * c_adv[b]) * (v0 + delta[so[3 * b]]))
            acc = acc + lam_b * self_
        out[row] = acc
    return out


def _dot32(a, b, order):
    """row dots of two fp32 [n, d] arrays, each product rounded: order 0 = numpy's pairwise sum, 1 = one chain from the last term"""
    prod = a * b
    if order == 0:
        return prod.sum(axis=1, dtype=np.float32)
    acc = np.zeros(len(a), dtype=np.float32)
    for k in range(a.shape[1] - 1, -1, -1):
        acc = acc + prod[:, k]
    return acc


def _sum32(v, order):
    v = np.asarray(v, dtype=np.float32)
    if order == 0:
        return v.sum(dtype=np.float32)
    acc = np.float32(0)
    for lo in range(0, len(v), 256):          # 256 terms in a chain, then the chains in a chain (the loss budget's ceil(B / 256))
        part = np.float32(0)
        for t in v[lo:lo + 256][::-1]:
            part = part + t
        acc = acc + part
    return acc


def step32(tab, u, i, j, U, lam, eps, adv_reg, order):
    """a plain fp32 numpy implementation in one of two summation orders: the chain of stages, each from its own predecessor.
    Order 0 walks steps 2 and 5 in key order (the kernel's bits), order 1 from a row's last incidence to its first."""
    tab = np.ascontiguousarray(tab, dtype=np.float32)
    pl = plan(u, i, j, U)
    nb, f = len(u), np.float32

    def coef(p, qi, qj):
        with np.errstate(over="ignore"):
            x = _dot32(p, qj, order) - _dot32(p, qi, order)
            sig = (f(1) / (f(1) + np.exp(-x))).astype(np.float32)
            sp = np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, f(20))))).astype(np.float32)
        return x, sig / f(nb), f(_sum32(sp, order)) / f(nb)

    p, qi, qj = tab[u], tab[U + i], tab[U + j]
    x, c, L = coef(p, qi, qj)
    sq = _dot32(p, p, order) + _dot32(qi, qi, order) + _dot32(qj, qj, order)
    out = {"plan": pl, "slot_of": pl["slot_of"], "x": x, "c": c, "L": float(L), "R": float(f(lam) * f(0.5) * _sum32(sq, order) / f(nb)), "L_adv": 0.0}
    if adv_reg != 0:
        G = walk_gamma32(tab, u, i, j, U, c, pl, reverse=order == 1)
        n = np.sqrt(_dot32(G, G, order))
        D = G * (f(eps) / np.maximum(n, f(TINY_NORM)))[:, None]
        rows = delta_rows_of(D, pl)
        xa, ca, La = coef(p + rows[0], qi + rows[1], qj + rows[2])
        out.update({"gamma": G, "norm": n, "delta": D, "x_adv": xa, "c_adv": ca, "L_adv": float(La)})
    out["grad"] = walk_grad32(tab, u, i, j, U, c, out.get("c_adv"), out.get("delta"), pl, lam, adv_reg, reverse=order == 1)
    return out


# ---------------------------------------------------------------- the checks
def _ratio(err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(np.max(r), nan=np.inf))


def _loss_budget(dx, nb, d, loss):
    return float(np.mean(dx)) + (math.ceil(nb / 256) + d + 32) * U32 * abs(loss)


def check_chain(tab, u, i, j, U, lam, eps, adv_reg, got, nb=None, budgets=None):
    """worst |error| / budget of every stage of `got` (x, c, L, R, and with adv_reg != 0 gamma, norm, delta, slot_of, x_adv, c_adv,
    L_adv; grad), each against the float64 restatement of that stage fed got's OWN earlier stages.  Exact stages (slot_of, the zero
    rows of delta, the untouched rows of grad) give 0 or inf.  budgets: a dict that receives {stage: (largest budget, largest
    magnitude)} for the condition test."""
    tab64 = np.asarray(tab, dtype=np.float64)
    d = tab64.shape[1]
    pl = plan(u, i, j, U)
    n_true = len(u) if nb is None else nb
    note = (lambda k, b, m: budgets.__setitem__(k, (float(np.max(b)), float(np.max(np.abs(m)))))) if budgets is not None else (lambda *a: None)
    r = {}
    one = coef64(tab64, u, i, j, U, lam, nb=n_true)
    dx = (d + 8) * U32 * one["S"]
    r["x"] = _ratio(np.abs(got["x"] - one["x"]), dx)
    r["c"] = _ratio(np.abs(got["c"] - one["c"]), (dx + 8 * U32) * one["c"])
    r["L"] = _ratio(abs(got["L"] - one["L"]), _loss_budget(dx, n_true, d, one["L"]))
    r["R"] = _ratio(abs(got["R"] - one["R"]), (math.ceil(n_true / 256) + d + 32) * U32 * one["R"])
    note("x", dx, one["x"]); note("c", (dx + 8 * U32) * one["c"], one["c"]); note("L", _loss_budget(dx, n_true, d, one["L"]), one["L"])
    note("R", (math.ceil(n_true / 256) + d + 32) * U32 * one["R"], one["R"])
    c_got = np.asarray(got["c"], dtype=np.float64)
    if adv_reg != 0:
        G, A = gamma64(tab64, u, i, j, U, c_got, pl)
        bG = (pl["n"][:, None] + 4) * U32 * A
        r["gamma"] = _ratio(np.abs(got["gamma"] - G), bG)
        G_got = np.asarray(got["gamma"], dtype=np.float64)
        n, D = delta64(G_got, eps)
        r["norm"] = _ratio(np.abs(got["norm"] - n), (d / 2 + 2) * U32 * n)
        r["delta"] = _ratio(np.abs(got["delta"] - D), (d / 2 + 5) * U32 * np.abs(D))
        zero = ~G_got.any(axis=1)
        if zero.any() and np.any(bits(np.asarray(got["delta"])[zero])):
            r["delta"] = math.inf                        # a zero row of Gamma: exact +0.0, never NaN
        r["slot_of"] = 0.0 if np.array_equal(np.asarray(got["slot_of"], dtype=np.int64), pl["slot_of"]) else math.inf
        D_got = np.asarray(got["delta"], dtype=np.float64)
        two = coef64(tab64, u, i, j, U, lam, delta_rows=delta_rows_of(D_got, pl), nb=n_true)
        dxa = (d + 10) * U32 * two["S"]
        r["x_adv"] = _ratio(np.abs(got["x_adv"] - two["x"]), dxa)
        r["c_adv"] = _ratio(np.abs(got["c_adv"] - two["c"]), (dxa + 8 * U32) * two["c"])
        r["L_adv"] = _ratio(abs(got["L_adv"] - two["L"]), _loss_budget(dxa, n_true, d, two["L"]))
        note("gamma", bG, G); note("norm", (d / 2 + 2) * U32 * n, n); note("delta", (d / 2 + 5) * U32 * np.abs(D), D)
        note("x_adv", dxa, two["x"]); note("c_adv", (dxa + 8 * U32) * two["c"], two["c"]); note("L_adv", _loss_budget(dxa, n_true, d, two["L"]), two["L"])
        g, Ag = grad64(tab64, u, i, j, U, c_got, np.asarray(got["c_adv"], dtype=np.float64), D_got, pl, lam, adv_reg, nb=n_true)
    else:
        g, Ag = grad64(tab64, u, i, j, U, c_got, None, None, pl, lam, 0.0, nb=n_true)
    nrow = np.zeros(len(tab64))
    nrow[pl["rows"]] = pl["n"]
    bg = (3 * nrow[:, None] + 8) * U32 * Ag
    r["grad"] = _ratio(np.abs(got["grad"] - g), bg)
    note("grad", bg, g)
    untouched = nrow == 0
    if np.any(bits(np.asarray(got["grad"], dtype=np.float32)[untouched])):
        r["grad"] = math.inf
    return r


# ---------------------------------------------------------------- the cases
DIMS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 128, 255, 256)
BATCHES = (1, 2, 63, 64, 65, 200, 1100)
# (d, B, kind): every d meets B = 65 and 200, every B meets d = 16 and 64; "hubs" plants the structures, "one_user" puts every triplet
# on one user (a run of B), "plain" draws everything (B < 200)
CASES = tuple(sorted({(d, B, "hubs" if B >= 200 else "plain") for d in DIMS for B in (65, 200)} |
                     {(d, B, "hubs" if B >= 200 else "plain") for d in (16, 64) for B in BATCHES})) + \
    ((16, 200, "one_user"), (64, 1100, "one_user"), (65, 200, "one_user"))
_SEEDS = {}                  # (d, B, kind) -> seed, where the default d * 10007 + B does not meet the condition on the table


def case(d, B, kind):
    """tab [N, d] fp32 ~ N(0, 1) / sqrt(d) per element (rows of norm about 1), triplets with i != j.  "hubs" (B >= 200): triplets 0
    and 1 with x = +40 / -40, on nodes the random triplets use too (a row touched by the x = -40 triplet alone would have a Gamma of
    1e-20, whose squares underflow: the budgets count roundings, not underflow; test_no_budget_is_vacuous holds every nonzero row's
    norm above 2^-40); triplets 2 and 3 on a user whose row is all zero, with four items no other triplet
    has (their Gamma is exactly zero); one node per entry of HUBS with exactly that many incidences in one role (roles in turn; an
    entry that does not fit the batch is left out); one item DUAL[0] times positive and DUAL[1] times negative; the rest random over
    the other nodes."""
    rng = np.random.default_rng(_SEEDS.get((d, B, kind), d * 10007 + B))
    U, I = N_USERS, N_ITEMS
    tab = (rng.standard_normal((U + I, d)) / math.sqrt(d)).astype(np.float32)
    hubs, zero_items = [], []
    if kind == "plain":
        u, i = rng.integers(0, U, B), rng.integers(0, I, B)
        j = (i + 1 + rng.integers(0, I - 1, B)) % I
    elif kind == "one_user":
        u, i = np.full(B, 7), rng.integers(0, I, B)
        j = (i + 1 + rng.integers(0, I - 1, B)) % I
        hubs.append((7, 0, B))
    else:
        free_u, free_i = list(rng.permutation(U)), list(rng.permutation(I))
        trip = np.full((3, B), -1, dtype=np.int64)
        zu = free_u.pop()
        for b in (2, 3):
            trip[:, b] = zu, free_i.pop(), free_i.pop()
            zero_items += [int(trip[1, b]), int(trip[2, b])]
        slots = [list(rng.permutation(np.arange(4, B))) for _ in range(3)]
        for k, count in enumerate(HUBS):
            role = k % 3
            if count > len(slots[role]) - 40:         # leave room for the others
                continue
            node = free_u.pop() if role == 0 else free_i.pop()
            for _ in range(count):
                trip[role, slots[role].pop()] = node
            hubs.append((int(node) + (U if role else 0), role, count))
        node = free_i.pop()
        taken = [slots[1].pop() for _ in range(DUAL[0])]
        rest = [s for s in slots[2] if s not in taken][:DUAL[1]]
        trip[1, taken], trip[2, rest] = node, node
        hubs += [(int(node) + U, 1, DUAL[0]), (int(node) + U, 2, DUAL[1])]
        pool_u, pool_i = np.array(free_u), np.array(free_i)
        for role, pool in ((0, pool_u), (1, pool_i), (2, pool_i)):
            todo = np.nonzero(trip[role] < 0)[0]
            trip[role, todo] = pool[rng.integers(0, len(pool), size=len(todo))]
        used_u = [x for x in pool_u if np.any(trip[0, 4:] == x)]          # nodes the random triplets touch: no row's Gamma is
        used_i = [x for x in pool_i if np.any(trip[1:, 4:] == x)]        # only as large as c at x = -40
        for b in (0, 1):
            trip[:, b] = used_u[b], used_i[2 * b], used_i[2 * b + 1]
        for b in np.nonzero(trip[1] == trip[2])[0]:       # two picks that met: one of them is from the pool
            k = 2 if trip[2, b] in pool_i else 1
            trip[k, b] = pool_i[(int(np.nonzero(pool_i == trip[k, b])[0][0]) + 1) % len(pool_i)]
        u, i, j = trip
        tab[zu] = 0
        for b, target in ((0, 40.0), (1, -40.0)):
            p = tab[u[b]].astype(np.float64)
            tab[u[b]] = (4 / math.sqrt((p * p).sum()) * p).astype(np.float32)       # norm 4: q_j - q_i = 2.5 p, whatever d is
            p = tab[u[b]].astype(np.float64)
            tab[U + j[b]] = (tab[U + i[b]].astype(np.float64) + target / (p * p).sum() * p).astype(np.float32)
    return {"d": d, "B": B, "kind": kind, "U": U, "I": I, "tab": tab, "u": np.asarray(u, dtype=np.int64), "i": np.asarray(i, dtype=np.int64),
            "j": np.asarray(j, dtype=np.int64), "hubs": hubs, "zero_items": zero_items, "lam": LAM, "eps": EPS, "adv_reg": ADV_REG}


_CACHE = {}


def named_case(d, B, kind):
    """case() and its float64 step, computed once and shared (nobody writes into them)"""
    key = (d, B, kind)
    if key not in _CACHE:
        c = case(d, B, kind)
        c["ref"] = step64(c["tab"], c["u"], c["i"], c["j"], c["U"], c["lam"], c["eps"], c["adv_reg"])
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def args(c):
    return c["tab"], c["u"], c["i"], c["j"], c["U"], c["lam"], c["eps"], c["adv_reg"]


# ---------------------------------------------------------------- training in float64 (the constructed push)
def adam64(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    m += (1 - b1) * (g - m)
    v *= b2
    v += (1 - b2) * g * g
    p -= lr / (1 - b1 ** t) * (m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps))


def sample_epoch(ptr, idx, n_items, rng):
    """one triplet per stored positive, the negative drawn until the user has not rated it; shuffled"""
    users = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    seen = np.zeros((len(ptr) - 1, n_items), dtype=bool)
    seen[users, idx] = True
    neg = rng.integers(0, n_items, len(idx))
    while True:
        bad = seen[users, neg]
        if not bad.any():
            break
        neg[bad] = rng.integers(0, n_items, int(bad.sum()))
    perm = rng.permutation(len(idx))
    return users[perm], idx[perm], neg[perm]


def train64(ptr, idx, n_items, d, epochs, adv_start, lam, eps, adv_reg, lr, batch, seed, init_std=0.01):
    """float64 training of the definition with the numpy sampler -> (tab [U + I, d], per-epoch means of (L, L', R))"""
    rng = np.random.default_rng(seed)
    U = len(ptr) - 1
    tab = init_std * rng.standard_normal((U + n_items, d))
    m, v, t, hist = np.zeros_like(tab), np.zeros_like(tab), 0, []
    for ep in range(epochs):
        u, i, j = sample_epoch(ptr, idx, n_items, rng)
        rows = []
        for lo in range(0, len(u), batch):
            sl = slice(lo, lo + batch)
            st = step64(tab, u[sl], i[sl], j[sl], U, lam, eps, adv_reg if ep >= adv_start else 0.0)
            t += 1
            adam64(tab, st["grad"], m, v, t, lr)
            rows.append((st["L"], st["L_adv"], st["R"]))
        hist.append(np.mean(rows, axis=0))
    return tab, np.array(hist)


# ---------------------------------------------------------------- replaying given epochs (the fidelity idiom of the GPU tests)
def adam32(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam in fp32, every operation rounded on its own, the coefficients from float64 (csrc/common.h, adam_elem)"""
    f = np.float32
    w1, w2 = f(1.0 - float(f(b1))), f(1.0 - float(f(b2)))
    step, bc2s = f(float(f(lr)) / (1.0 - float(f(b1)) ** t)), f(math.sqrt(1.0 - float(f(b2)) ** t))
    m[...] = m + w1 * (g - m)
    v[...] = v * f(b2) + w2 * g * g
    p[...] = p - step * (m / (np.sqrt(v) / bc2s + f(eps)))


def replay(tab0, epochs, batch, U, lam, eps, adv_reg, adv_start, lr, fp32, opt="adam", done=0, order=0):
    """train from tab0 over the given epochs of triplets [(u, i, j), ...]: float64, or the plain fp32 numpy implementation (step32
    in the given summation order, with the walks in key order) -> (table, per-epoch means of (L, L', R))"""
    tab = np.array(tab0, dtype=np.float32 if fp32 else np.float64)
    m, v, t, hist = np.zeros_like(tab), np.zeros_like(tab), 0, []
    for ep, (u, i, j) in enumerate(epochs):
        adv, rows = (adv_reg if done + ep >= adv_start else 0.0), []
        for lo in range(0, len(u), batch):
            sl = slice(lo, lo + batch)
            st = step32(tab, u[sl], i[sl], j[sl], U, lam, eps, adv, order) if fp32 else step64(tab, u[sl], i[sl], j[sl], U, lam, eps, adv)
            t += 1
            if opt == "sgd":
                tab = tab - (np.float32(lr) * st["grad"] if fp32 else float(np.float32(lr)) * st["grad"])
            else:
                (adam32 if fp32 else adam64)(tab, st["grad"], m, v, t, lr)
            rows.append((st["L"], st["L_adv"], st["R"]))
        hist.append(np.mean(np.array(rows, dtype=np.float64), axis=0))
    return tab, np.array(hist)
