"""NumPy restatement of the Mult-VAE victim's train step (include/recad_hip.h, "Mult-VAE victim"; csrc/multvae.hip): every stage
from that stage's own inputs in a chosen precision (float64 is the reference; plain float32 in two summation orders is what the
budgets are sized for), the fp32 walks the kernels must reproduce to the bit (the sparse layer, the k-ordered chains through the
oracle, the bias sums, the tanh backward, gW1, Adam through the oracle), the keep masks and the noise exactly as the library
draws them, the rounding budgets of the tolerant stages, and the table of cases the host and the GPU tests share.  No GPU, no torch.

A budget counts the fp32 roundings a correct implementation may make: (roundings) x 2^-24 x (sum of the magnitudes they act on).
The device evaluates its transcendental stages in double and rounds once, so it uses a small part of them; the float64
evaluation's own error (a few 2^-53 of the same magnitudes) is added as 2^-40 of the budget's magnitude sum."""
import math

import numpy as np

from ._drop_restate import _drop_keep, _mix64, _step_seed

R24 = 2.0 ** -24
F64_SLACK = 2.0 ** -40
SENTINEL = 7.0
EPS_STREAM = 0xA5A5A5A5A5A5A5A5
HASH_MUL = 0xD1342543DE82EF95
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shapes(I, H, L):
    return (("W1", (I, H)), ("b1", (H,)), ("W2", (2 * L, H)), ("b2", (2 * L,)), ("W3", (H, L)), ("b3", (H,)), ("W4", (I, H)), ("b4", (I,)))


def split(theta, I, H, L):
    """views of the flat buffer, in its order"""
    out, at = {}, 0
    for name, shape in shapes(I, H, L):
        n = int(np.prod(shape))
        out[name] = theta[at:at + n].reshape(shape)
        at += n
    assert at == theta.size
    return out


def n_params(I, H, L):
    return sum(int(np.prod(s)) for _, s in shapes(I, H, L))


def beta_at(step, cap, total):
    cap = float(f32(cap))
    return min(cap, step / total) if total > 0 else cap


# ---------------------------------------------------------------- integer draws, exactly
def keep_masks(seed, step, users, rows, dropout):
    """per batch row, the keep decision of each stored item (bool)"""
    keep_prob = 1.0 - float(f32(dropout))
    s = _step_seed(seed, step)
    return [_drop_keep(_step_seed(s, int(u)), int(r.max()) + 1, keep_prob)[r] for u, r in zip(users, rows)]


def c_of(n, dropout):
    """c_u = n^-1/2 / keep in double, rounded once"""
    return f32(1.0 / np.sqrt(np.asarray(n, dtype=np.float64)) / (1.0 - float(f32(dropout))))


def eps64(seed, step, users, L):
    """the standard normals in float64, before their rounding to fp32"""
    s = _step_seed(seed ^ EPS_STREAM, step)
    out = np.empty((len(users), L))
    with np.errstate(over="ignore"):
        t = np.arange(2 * L, dtype=np.uint64) * np.uint64(HASH_MUL)
        for b, u in enumerate(users):
            r = _mix64(np.uint64(_step_seed(s, int(u))) ^ t)
            u1 = ((r[0::2] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
            u2 = (r[1::2] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
            out[b] = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    return out


# ---------------------------------------------------------------- the stages, each from its own inputs, in precision dt
def _sum(x, axis, order):
    """a sum in the array's own precision: numpy's pairwise order, or the same over the reversed axis"""
    return np.sum(x if order == 0 else np.flip(x, axis=axis), axis=axis, dtype=x.dtype)


def st_a(W1, rows, masks, dt=np.float64, order=0):
    W1 = W1.astype(dt)
    return np.stack([_sum(W1[r[m]], 0, order) if m.any() else np.zeros(W1.shape[1], dt) for r, m in zip(rows, masks)])


def st_pre1(c, a, b1, dt=np.float64):
    return c.astype(dt)[:, None] * a.astype(dt) + b1.astype(dt)


def st_tanh(pre, dt=np.float64):
    return np.tanh(pre.astype(dt))


def st_lin(x, W, b=None, dt=np.float64, order=0):
    """x [M, K] . W [N, K]^T (+ b)"""
    x, W = x.astype(dt), W.astype(dt)
    y = x @ W.T if order == 0 else x[:, ::-1] @ W[:, ::-1].T
    return y if b is None else y + b.astype(dt)


def st_z(mu, lv, eps, dt=np.float64):
    return mu.astype(dt) + eps.astype(dt) * np.exp(dt(0.5) * lv.astype(dt))


def st_kl(mu, lv, dt=np.float64, order=0):
    mu, lv = mu.astype(dt), lv.astype(dt)
    return dt(-0.5) * _sum(((dt(1) + lv) - mu * mu) - np.exp(lv), 1, order)


def st_lse(logits, dt=np.float64, order=0):
    l = logits.astype(dt)
    mx = l.max(axis=1)
    return mx + np.log(_sum(np.exp(l - mx[:, None]), 1, order))


def st_nll(logits, lse, rows, dt=np.float64, order=0):
    l, lse = logits.astype(dt), lse.astype(dt)
    return np.array([_sum(lse[b] - l[b, r], 0, order) for b, r in enumerate(rows)], dtype=dt)


def st_loss(nll, kl, beta, dt=np.float64, order=0, b_div=None):
    B = dt(len(nll) if b_div is None else b_div)
    return _sum(nll.astype(dt) + dt(beta) * kl.astype(dt), 0, order) / B


def st_dl(logits, lse, rows, dt=np.float64, b_div=None, with_n=True):
    l, lse = logits.astype(dt), lse.astype(dt)
    B = dt(l.shape[0] if b_div is None else b_div)
    n = np.array([len(r) if with_n else 1 for r in rows], dtype=dt)
    x = np.zeros(l.shape, dt)
    for b, r in enumerate(rows):
        x[b, r] = 1
    return (n[:, None] * np.exp(l - lse[:, None]) - x) / B


def st_tanh_bwd(dh, h, dt=np.float64):
    dh, h = dh.astype(dt), h.astype(dt)
    return dh * (dt(1) - h * h)


def st_dml(dz, mu, lv, eps, beta, dt=np.float64, b_div=None):
    dz, mu, lv, eps = (x.astype(dt) for x in (dz, mu, lv, eps))
    B = dz.shape[0] if b_div is None else b_div
    cb, cb2 = dt(beta / B), dt(beta / (2.0 * B))
    return np.concatenate([dz + cb * mu, dt(0.5) * dz * eps * np.exp(dt(0.5) * lv) + cb2 * (np.exp(lv) - dt(1))], axis=1)


def st_gw1(c, dp1, rows, masks, I, dt=np.float64, order=0):
    g = np.zeros((I, dp1.shape[1]), dt)
    order_b = range(len(rows)) if order == 0 else range(len(rows) - 1, -1, -1)
    for b in order_b:
        g[rows[b][masks[b]]] += dt(c[b]) * dp1[b].astype(dt)
    return g


# ---------------------------------------------------------------- budgets of the tolerant stages (float64 from the same inputs)
def _with_slack(b, mag):
    return b + F64_SLACK * mag + 2.0 ** -149


def bud_tanh(pre):
    """3 roundings of the result (an fp32 tanh within one ulp, and the store)"""
    h = np.abs(np.tanh(pre.astype(np.float64)))
    return _with_slack(3 * R24 * h, h)


def bud_z(mu, lv, eps):
    """exp (2), the product, the sum: 4 roundings on |mu| + |eps sigma|"""
    mag = np.abs(mu.astype(np.float64)) + np.abs(eps.astype(np.float64)) * np.exp(0.5 * lv.astype(np.float64))
    return _with_slack(4 * R24 * mag, mag)


def bud_kl(mu, lv):
    """per term 6 roundings (1 + lv, mu^2, the difference, exp twice, the difference), then L - 1 adds and the factor"""
    mu, lv = mu.astype(np.float64), lv.astype(np.float64)
    mag = 0.5 * np.sum(1.0 + np.abs(lv) + mu * mu + np.exp(lv), axis=1)
    return _with_slack((mu.shape[1] + 6) * R24 * mag, mag)


def bud_lse(logits):
    """the argument's rounding moves exp by |l - max| roundings (softmax-weighted), exp 2, I - 1 adds; log 2; the last add 1"""
    l = logits.astype(np.float64)
    mx = l.max(axis=1, keepdims=True)
    e = np.exp(l - mx)
    s = e.sum(axis=1)
    d_eff = (e * np.abs(l - mx)).sum(axis=1) / s
    mag = (l.shape[1] + 2 + d_eff) + 2 * np.abs(np.log(s)) + np.abs(mx[:, 0] + np.log(s))
    return _with_slack(R24 * mag, mag)


def bud_nll(logits, lse, rows):
    """per term one rounding, then n - 1 adds"""
    l = logits.astype(np.float64)
    mag = np.array([np.sum(np.abs(lse[b] - l[b, r])) for b, r in enumerate(rows)])
    n = np.array([len(r) for r in rows])
    return _with_slack((n + 1) * R24 * mag, mag)


def bud_loss(nll, kl, beta, b_div=None):
    B = len(nll) if b_div is None else b_div
    mag = float(np.sum(np.abs(nll) + beta * np.abs(kl))) / B
    return _with_slack((len(nll) + 3) * R24 * mag, mag)


def bud_dl(logits, lse, rows, b_div=None):
    """the argument's rounding (|l - lse| roundings of p), exp 2, n p 1 on n p; the difference and the division on the result"""
    l = logits.astype(np.float64)
    B = l.shape[0] if b_div is None else b_div
    n = np.array([len(r) for r in rows], dtype=np.float64)[:, None]
    npk = n * np.exp(l - lse[:, None])
    val = np.abs(st_dl(logits, lse, rows, b_div=b_div))
    mag = (np.abs(l - lse[:, None]) + 3) * npk / B + 2 * val
    return _with_slack(R24 * mag, mag)


def bud_dml(dz, mu, lv, eps, beta, b_div=None):
    dz, mu, lv, eps = (x.astype(np.float64) for x in (dz, mu, lv, eps))
    B = dz.shape[0] if b_div is None else b_div
    cb, cb2 = beta / B, beta / (2.0 * B)
    m1 = np.abs(dz) + cb * np.abs(mu)
    m2 = np.abs(0.5 * dz * eps * np.exp(0.5 * lv)) + cb2 * (np.exp(lv) + 1.0)
    return np.concatenate([_with_slack(3 * R24 * m1, m1), _with_slack(6 * R24 * m2, m2)], axis=1)


def ratio(got, want, budget):
    """worst |got - want| / budget; inf when something is not finite"""
    got, want, budget = (np.asarray(x, dtype=np.float64) for x in (got, want, budget))
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(want))):
        return float("inf")
    return float(np.max(np.abs(got - want) / budget)) if got.size else 0.0


# ---------------------------------------------------------------- the fp32 walks: what the kernels reproduce to the bit
def chain(A, B, bias=None):
    """C[m, n] = the k-ordered chain s = fmaf(A[m, k], B[n, k], s) from +0.0 (the oracle's orc_score_rows), + bias[n] by one fp32 add"""
    from oracle import oracle as orc

    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    if A.shape[1] == 0:
        y = np.zeros((A.shape[0], B.shape[0]), np.float32)
    else:
        y = orc.score_rows(A, B)
    return y if bias is None else y + np.asarray(bias, dtype=np.float32)


def a_walk(W1, rows, masks, descending=False):
    out = np.zeros((len(rows), W1.shape[1]), np.float32)
    for b, (r, m) in enumerate(zip(rows, masks)):
        acc = np.zeros(W1.shape[1], np.float32)
        for i in (r[m][::-1] if descending else r[m]):
            acc = acc + W1[i]
        out[b] = acc
    return out


def pre1_walk(c, a, b1):
    return (c.astype(np.float32)[:, None] * a.astype(np.float32)) + b1.astype(np.float32)


def colsum_walk(x):
    acc = np.zeros(x.shape[1], np.float32)
    for r in range(x.shape[0]):
        acc = acc + x[r].astype(np.float32)
    return acc


def tanh_bwd_walk(dh, h):
    t = h * h
    s = f32(1) - t
    return dh * s


def gw1_walk(c, dp1, rows, masks, I, descending=False):
    """row i: acc = fmaf(c_u, dp1[u, h], acc) over the batch positions that hold i as a kept entry, ascending"""
    holders = [[] for _ in range(I)]
    for b, (r, m) in enumerate(zip(rows, masks)):
        for i in r[m]:
            holders[int(i)].append(b)
    g = np.zeros((I, dp1.shape[1]), np.float32)
    for i, hs in enumerate(holders):
        if hs:
            hs = hs[::-1] if descending else hs
            g[i] = chain(np.asarray(c, np.float32)[hs][None, :], np.ascontiguousarray(dp1[hs].T))[0]
    return g


def adam_oracle(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """in place, through the oracle's orc_adam"""
    from oracle import oracle as orc

    orc.adam(p, np.ascontiguousarray(g, dtype=np.float32), m, v, t, lr, b1, b2, eps)


def grads_walk(P, s, rows, masks, I):
    """the flat gradient by the fp32 walks, from the stages `s` (dl, h2, dp2, z, dml, h1, dp1, c)"""
    g = {"W4": chain(s["dl"].T, s["h2"].T), "b4": colsum_walk(s["dl"]), "W3": chain(s["dp2"].T, s["z"].T), "b3": colsum_walk(s["dp2"]),
         "W2": chain(s["dml"].T, s["h1"].T), "b2": colsum_walk(s["dml"]), "W1": gw1_walk(s["c"], s["dp1"], rows, masks, I),
         "b1": colsum_walk(s["dp1"])}
    return np.concatenate([g[k].reshape(-1) for k in NAMES])


# ---------------------------------------------------------------- a whole step in one precision (chained), with the wrong variants
VARIANTS = ("no_inv_keep", "l1_norm", "dl_without_n", "nll_kept_only", "softmax_masks_seen", "kl_sign", "dlogvar_without_half",
            "beta_on_nll", "tanh_prime_at_pre", "gw1_ignores_mask", "full_batch_divisor", "sample_at_inference")


def step(P, rows, masks, eps, dropout, beta, dt=np.float64, order=0, variant=None, train=True, b_div=None, full_batch=None):
    """Every stage of one step, each from the stage before it, in precision dt.  train = False: inference (no dropout, z = mu).
    `variant` names one deliberate mistake (VARIANTS)."""
    I, L = P["W4"].shape[0], P["W3"].shape[1]
    keep = 1.0 - float(f32(dropout)) if train else 1.0
    n = np.array([len(r) for r in rows], dtype=np.float64)
    if not train:
        masks = [np.ones(len(r), bool) for r in rows]
    s = {}
    with np.errstate(divide="ignore"):
        norm = np.where(n > 0, 1.0 / n if variant == "l1_norm" else 1.0 / np.sqrt(n), 0.0)
    s["c"] = (norm / (1.0 if variant == "no_inv_keep" else keep)).astype(np.float32)
    s["a"] = st_a(P["W1"], rows, masks, dt, order)
    s["pre1"] = st_pre1(s["c"], s["a"], P["b1"], dt)
    s["h1"] = st_tanh(s["pre1"], dt)
    if not train and variant != "sample_at_inference":
        s["ml"] = st_lin(s["h1"], P["W2"][:L], P["b2"][:L], dt, order)
        s["z"] = s["ml"]
    else:
        s["ml"] = st_lin(s["h1"], P["W2"], P["b2"], dt, order)
        mu, lv = s["ml"][:, :L], s["ml"][:, L:]
        s["z"] = st_z(mu, lv, eps, dt)
        s["kl"] = st_kl(mu, lv, dt, order) * (-1 if variant == "kl_sign" else 1)
    s["pre2"] = st_lin(s["z"], P["W3"], P["b3"], dt, order)
    s["h2"] = st_tanh(s["pre2"], dt)
    s["logits"] = st_lin(s["h2"], P["W4"], P["b4"], dt, order)
    if not train:
        return s
    if variant == "full_batch_divisor":
        b_div = full_batch
    lg = s["logits"]
    if variant == "softmax_masks_seen":
        lg = lg.copy()
        for b, r in enumerate(rows):
            lg[b, r] = -np.inf
    s["lse"] = st_lse(lg, dt, order)
    nll_rows = [r[m] for r, m in zip(rows, masks)] if variant == "nll_kept_only" else rows
    s["nll"] = st_nll(s["logits"], s["lse"], nll_rows, dt, order)
    if variant == "beta_on_nll":
        s["loss"] = st_loss(dt(beta) * s["nll"], s["kl"], 1.0, dt, order, b_div)
    else:
        s["loss"] = st_loss(s["nll"], s["kl"], beta, dt, order, b_div)
    s["dl"] = st_dl(s["logits"], s["lse"], rows, dt, b_div, with_n=variant != "dl_without_n")
    s["dh2"] = st_lin(s["dl"], P["W4"].T, None, dt, order)
    s["dp2"] = st_tanh_bwd(s["dh2"], s["pre2"] if variant == "tanh_prime_at_pre" else s["h2"], dt)
    s["dz"] = st_lin(s["dp2"], P["W3"].T, None, dt, order)
    s["dml"] = st_dml(s["dz"], mu, lv, eps, beta, dt, b_div)
    if variant == "kl_sign":
        s["dml"] = st_dml(s["dz"], mu, lv, eps, -beta, dt, b_div)
    if variant == "dlogvar_without_half":
        s["dml"][:, L:] += dt(0.5) * s["dz"] * eps.astype(dt) * np.exp(dt(0.5) * lv)
    s["dh1"] = st_lin(s["dml"], P["W2"].T, None, dt, order)
    s["dp1"] = st_tanh_bwd(s["dh1"], s["pre1"] if variant == "tanh_prime_at_pre" else s["h1"], dt)
    gm = [np.ones(len(r), bool) for r in rows] if variant == "gw1_ignores_mask" else masks
    g = {"W4": st_lin(s["dl"].T, s["h2"].T, None, dt, order), "b4": _sum(s["dl"], 0, order),
         "W3": st_lin(s["dp2"].T, s["z"].T, None, dt, order), "b3": _sum(s["dp2"], 0, order),
         "W2": st_lin(s["dml"].T, s["h1"].T, None, dt, order), "b2": _sum(s["dml"], 0, order),
         "W1": st_gw1(s["c"], s["dp1"], rows, gm, I, dt, order), "b1": _sum(s["dp1"], 0, order)}
    s["grad"] = np.concatenate([g[k].reshape(-1) for k in NAMES])
    return s


TOLERANT = ("h1", "z", "kl", "h2", "lse", "nll", "loss", "dl", "dml")


def tolerant_ratios(got, P, rows, eps, beta, b_div=None):
    """worst err / budget of every tolerant stage of `got`, each restated in float64 from got's OWN inputs of that stage"""
    L = P["W3"].shape[1]
    g = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    mu, lv = g["ml"][:, :L], g["ml"][:, L:]
    return {
        "h1": ratio(g["h1"], st_tanh(g["pre1"]), bud_tanh(g["pre1"])),
        "z": ratio(g["z"], st_z(mu, lv, eps), bud_z(mu, lv, eps)),
        "kl": ratio(g["kl"], st_kl(mu, lv), bud_kl(mu, lv)),
        "h2": ratio(g["h2"], st_tanh(g["pre2"]), bud_tanh(g["pre2"])),
        "lse": ratio(g["lse"], st_lse(g["logits"]), bud_lse(g["logits"])),
        "nll": ratio(g["nll"], st_nll(g["logits"], g["lse"], rows), bud_nll(g["logits"], g["lse"], rows)),
        "loss": ratio(g["loss"], st_loss(g["nll"], g["kl"], beta, b_div=b_div), bud_loss(g["nll"], g["kl"], beta, b_div)),
        "dl": ratio(g["dl"], st_dl(g["logits"], g["lse"], rows, b_div=b_div), bud_dl(g["logits"], g["lse"], rows, b_div)),
        "dml": ratio(g["dml"], st_dml(g["dz"], mu, lv, eps, beta, b_div=b_div), bud_dml(g["dz"], mu, lv, eps, beta, b_div)),
    }


def budget_caps(got, P, rows, eps, beta):
    """largest budget / largest value of each tolerant stage (the host test holds them below 2^-10)"""
    L = P["W3"].shape[1]
    g = {k: np.asarray(v, dtype=np.float64) for k, v in got.items()}
    mu, lv = g["ml"][:, :L], g["ml"][:, L:]
    b = {"h1": bud_tanh(g["pre1"]), "z": bud_z(mu, lv, eps), "kl": bud_kl(mu, lv), "h2": bud_tanh(g["pre2"]), "lse": bud_lse(g["logits"]),
         "nll": bud_nll(g["logits"], g["lse"], rows), "loss": bud_loss(g["nll"], g["kl"], beta), "dl": bud_dl(g["logits"], g["lse"], rows),
         "dml": bud_dml(g["dz"], mu, lv, eps, beta)}
    top = {k: float(np.max(np.abs(g[k]))) for k in b}
    # dl is a difference that cancels to exactly 0 when a row is the whole catalogue of one item: its minuend n p / B stands in
    n = np.array([len(r) for r in rows], dtype=np.float64)[:, None]
    top["dl"] = max(top["dl"], float(np.max(n * np.exp(g["logits"] - g["lse"][:, None]))) / len(rows))
    return {k: float(np.max(v)) / max(top[k], 2.0 ** -126) for k, v in b.items()}


# ---------------------------------------------------------------- the cases
# (I, H, L, B, the batch rows' lengths (cycled, clipped to I), dropout, anneal_cap, special)
_TABLE = [
    (1, 1, 1, 1, (1,), 0.0, 0.0, None), (2, 3, 2, 2, (1, 2), 0.5, 0.2, None), (3, 1, 1, 1, (2,), 0.0, 0.2, None),
    (3, 16, 2, 2, (1, 2, 3), 0.5, 0.0, "full_user"), (63, 3, 1, 2, (1, 2, 63), 0.5, 0.2, "full_user"), (64, 16, 16, 63, (2, 64, 1), 0.0, 0.2, None),
    (65, 64, 2, 64, (63, 64, 65), 0.5, 0.2, "full_user"), (127, 65, 33, 65, (1, 2, 63, 65), 0.5, 0.0, None),
    (128, 130, 16, 1, (64,), 0.5, 0.2, None), (129, 16, 1, 2, (65, 1), 0.0, 0.0, None), (200, 64, 16, 200, (1, 2, 63, 64, 65, 197), 0.5, 0.2, None),
    (300, 65, 33, 63, (197, 2, 1, 64), 0.5, 0.2, None), (1100, 130, 33, 200, (1, 2, 63, 64, 65, 197), 0.5, 0.2, None),
    (1100, 16, 2, 2, (1100, 197), 0.0, 0.2, "full_user"), (300, 1, 1, 64, (1, 2), 0.5, 0.2, "all_dropped"), (200, 3, 2, 65, (2, 1), 0.5, 0.0, "all_dropped"),
    (128, 16, 16, 63, (63, 64), 0.5, 0.2, "logit40"), (65, 64, 2, 2, (1, 65), 0.0, 0.2, "logit40"), (300, 130, 33, 2, (197,), 0.5, 0.0, "logit40"),
    (127, 16, 16, 64, (2, 63), 0.5, 0.2, "logvar20"), (64, 65, 2, 65, (64,), 0.0, 0.2, "logvar20"), (200, 3, 33, 1, (197,), 0.5, 0.2, "logvar20"),
    (129, 64, 16, 63, (65, 2), 0.5, 0.2, "zeroW4"), (3, 3, 1, 2, (1,), 0.0, 0.0, "zeroW4"), (300, 16, 2, 200, (1, 63), 0.5, 0.2, "zeroW4"),
    (2, 1, 1, 200, (1, 2), 0.5, 0.2, None), (63, 130, 1, 64, (1,), 0.0, 0.2, None), (65, 1, 33, 65, (2, 65), 0.5, 0.2, None),
    (127, 3, 16, 200, (63,), 0.5, 0.0, None), (128, 64, 33, 2, (128, 1), 0.5, 0.2, "full_user"), (129, 65, 2, 1, (1,), 0.5, 0.2, None),
    (200, 130, 1, 63, (197, 64), 0.0, 0.0, None), (300, 64, 16, 65, (65, 63, 2), 0.5, 0.2, None), (1100, 3, 1, 1, (197,), 0.5, 0.2, None),
    (1100, 65, 16, 64, (64, 1, 197), 0.5, 0.0, None), (64, 130, 33, 200, (2, 1, 63), 0.0, 0.2, None), (1, 16, 2, 63, (1,), 0.5, 0.2, None),
    (3, 64, 1, 65, (3, 1, 2), 0.5, 0.2, "full_user"), (63, 65, 16, 1, (63,), 0.0, 0.2, "full_user"), (65, 130, 2, 200, (65, 64), 0.5, 0.2, None),
]
CASES = [(f"c{k:02d}-I{t[0]}-H{t[1]}-L{t[2]}-B{t[3]}" + (f"-{t[7]}" if t[7] else ""), t) for k, t in enumerate(_TABLE)]
TOTAL_ANNEAL = 10


def make_case(k):
    """Case k: a rating CSR over U = B + 2 users (the last two are not in the batch; one batch position repeats user 0 when B > 2),
    the batch's user ids, the parameters, and the step count at which beta reaches the case's cap (or 0 for beta = 0)."""
    name, (I, H, L, B, lens, dropout, cap, special) = CASES[k]
    rng = np.random.default_rng(1000 + k)
    U = B + 2
    absent = (I - 1) // 2 if I >= 3 else None            # an item nobody in the batch has (but for a user who has every item)
    pool = np.array([i for i in range(I) if i != absent])
    rows = []
    for u in range(U):
        n = min(lens[u % len(lens)], I)
        if n == I and special == "full_user":
            rows.append(np.arange(I))
        else:
            rows.append(np.sort(rng.choice(pool, size=min(n, len(pool)), replace=False)))
    users = rng.permutation(B).astype(np.int32)
    if B > 2:
        users[-1] = users[0]                              # a repeated user
    if special == "full_user":
        rows[users[B // 2]] = np.arange(I)                # a user of the batch who has every item
    ptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    P = {}
    for nm, shape in shapes(I, H, L):
        fan = shape[1] if len(shape) == 2 and nm != "W1" else 1
        scale = (1.0 / math.sqrt(fan)) if len(shape) == 2 else 0.1
        P[nm] = (rng.standard_normal(shape) * scale).astype(np.float32)
    if special == "logit40" and I >= 2:
        P["b4"][0], P["b4"][1] = 40.0, -40.0
    if special == "logvar20":
        P["b2"][L] = 20.0
        if L > 1:
            P["b2"][L + 1] = -20.0
    if special == "zeroW4":
        P["W4"][:] = 0.0
    theta = np.concatenate([P[nm].reshape(-1) for nm in NAMES])
    seed = 77 + k
    step0 = TOTAL_ANNEAL * 3 if cap > 0 else 0             # past the anneal: beta = cap; 0: beta = 0
    brows = [rows[u] for u in users]
    if special == "all_dropped":                           # a step at which some item of the batch loses every entry
        for step0 in range(step0, step0 + 4096):
            masks = keep_masks(seed, step0, users, brows, dropout)
            had, kept = np.zeros(I, bool), np.zeros(I, bool)
            for r, m in zip(brows, masks):
                had[r] = True
                kept[r[m]] = True
            if (had & ~kept).any():
                break
        else:
            raise AssertionError("no step drops every entry of an item")
    return dict(name=name, I=I, H=H, L=L, B=B, U=U, ptr=ptr, col=col, users=users, rows=brows, theta=theta, dropout=dropout, cap=cap,
                total=TOTAL_ANNEAL, step0=step0, seed=seed, special=special, absent=absent,
                beta=beta_at(step0, cap, TOTAL_ANNEAL))


# ---------------------------------------------------------------- training in float64 (the constructed push) and replays
def adam64(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    m += (1 - b1) * (g - m)
    v *= b2
    v += (1 - b2) * g * g
    p -= lr / (1 - b1 ** t) * (m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps))


def adam32(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam in fp32, every operation rounded on its own, the coefficients from float64 (csrc/common.h, adam_elem)"""
    f = np.float32
    w1, w2 = f(1.0 - float(f(b1))), f(1.0 - float(f(b2)))
    stp, bc2s = f(float(f(lr)) / (1.0 - float(f(b1)) ** t)), f(math.sqrt(1.0 - float(f(b2)) ** t))
    m[...] = m + w1 * (g - m)
    v[...] = v * f(b2) + w2 * g * g
    p[...] = p - stp * (m / (np.sqrt(v) / bc2s + f(eps)))


def replay(theta0, ptr, col, I, H, L, epochs_users, batch, seed, dropout, cap, total, lr, dt=np.float64, step0=0, opt="adam"):
    """The training the library runs on the given epochs (each an order of user ids), chained in precision dt with the library's
    masks and noise (eps rounded to fp32, as the library stores it); opt = "sgd": p -= lr g.  Returns (theta, [per step loss])."""
    theta = theta0.astype(dt).copy()
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    t, losses = step0, []
    for users in epochs_users:
        for s0 in range(0, len(users), batch):
            us = users[s0:s0 + batch]
            rows = [col[ptr[u]:ptr[u + 1]].astype(np.int64) for u in us]
            masks = keep_masks(seed, t, us, rows, dropout)
            eps = eps64(seed, t, us, L).astype(np.float32)
            s = step(split(theta, I, H, L), rows, masks, eps, dropout, beta_at(t, cap, total), dt=dt)
            if opt == "sgd":
                theta -= dt(lr) * s["grad"].astype(dt)
            else:
                (adam64 if dt == np.float64 else adam32)(theta, s["grad"].astype(dt), m, v, t + 1, lr)
            losses.append(float(s["loss"]))
            t += 1
    return theta, losses


def scores64(theta, ptr, col, I, H, L, users):
    P = split(np.asarray(theta, dtype=np.float64), I, H, L)
    rows = [col[ptr[u]:ptr[u + 1]].astype(np.int64) for u in users]
    return step(P, rows, None, None, 0.0, 0.0, train=False)["logits"]
