"""float64 numpy restatement of the AIA surrogate's device operations (csrc/aia.hip), for the tests: one WMF / Adam step, the
adjoint of one step (the two reverse launches), the attack loss with its gradient, project and the G step -- and beside each
value a first-order bound on the error of the fp32 kernels.  It is written from the formulas (the comments of aia.hip and
include/recad_hip.h); nothing here is the product's code path, and tests/test_aia_host.py checks it against torch autograd.
It follows tests/_aush_restate.py and shares that module's constants, comparison and Adam bound.

Layout.  A state tensor is [(R + I), dpad]: R user rows (n_real real ones, then the fake ones), then I item rows; columns
d .. dpad - 1 are 0.  The functions take and return that shape; inputs are the device's own fp32 values (or float64, when a test
chains steps without rounding).

Error bounds.  u = 2^-24.  A dot product of n terms is within (n + 2) u sum |a_i b_i| of the exact one in any summation order
(n = dpad: the xor butterfly of the step kernels and the fma chain of the loss kernels alike).  A sum of c terms accumulates
(c + 2) u sum |t_i| on top of its terms' own bounds; a P row of the step kernels is summed in 256 / dpad strided parts that
are then added, so c grows by 256 / dpad.  Adam goes through _aush_restate.adam_ref with the gradient's bound.  The adjoint of
Adam is a handful of fp32 operations per element: the count of roundings on each term times u.  expf / logf enter with K ulps
of their result: K_ULP where every expf argument lies in [-20, 20] (asserted here), K_EXP_WIDE for the one overflow case, whose
arguments reach down to EXP_WIDE_LO.  An expf result below the smallest normal number is taken to be within K ulps of THAT
number (absolute), so an underflowing or flushed term costs nothing visible.  Everything is first order.

The attack loss is discontinuous where s_ui crosses s_ut, so it has no bound there: attack_loss_ref refuses (AssertionError) an
input with a pair (u, i != t) whose two scores differ but by less than their bounds; exact fp32 ties (i's Q row a copy of t's)
are equal here too and are masked in, as `>=` says."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

from ._aush_restate import K_ULP, U24, adam_consts, adam_ref, capped, within  # noqa: F401  (re-exported for the tests)

FLT_MIN = float(np.finfo(np.float32).tiny)
# The overflow case of the attack loss (scores above 90) shifts every expf argument by the running maximum, so they are all
# <= 0 but reach far below the [-20, 20] on which K_ULP was measured.  Measured the same way on an MI355X against fp64 (a kernel
# of one expf per thread, built with the library's flags): 2^22 arguments on [EXP_WIDE_LO, 0], half on a grid and half random, the
# error in ulps of max(|result|, FLT_MIN).  The largest was 1.00, at x = -103.279 where the result is subnormal (subnormal results
# are returned, not flushed: each is the nearest or the next subnormal); over the normal results it was 0.83.  The same program
# gives 0.84 on [-20, 20], the figure K_ULP was built from.  K_EXP_WIDE is twice the largest, as K_ULP is twice its own.
EXP_WIDE_LO = -256.0
EXP_WIDE_MEASURED = 1.00
K_EXP_WIDE = 2 * EXP_WIDE_MEASURED

FLAWS = ("no_wd_gbar", "xbar_no_w", "first_block_only", "strict_tie", "factor2")


def f32(a):
    return float(np.float32(a))


def dpad_of(d):
    return 16 if d <= 16 else (32 if d <= 32 else 64)


def batch_rows(c, perm, j):
    s0 = j * c.batch
    return np.asarray(perm[s0:min(s0 + c.batch, c.R)], dtype=np.int64)


def _state(c, a):
    return np.asarray(a, dtype=np.float64).reshape(c.R + c.I, c.dpad)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------- the batch part of one step's gradient
def _batch_entries(c, th, rows):
    """The stored entries of the batch's rows: index k, position of the row in the batch, the two state rows, the residual
    e = X - p . q with its bound, and the weight (w_pos where X > 0, else 0)."""
    rowptr, col, x = np.asarray(c.rowptr, dtype=np.int64), np.asarray(c.col, dtype=np.int64), np.asarray(c.x, dtype=np.float64)
    lens = rowptr[rows + 1] - rowptr[rows]
    k = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    bpos = np.repeat(np.arange(len(rows)), lens)
    r, ci = rows[bpos], c.R + col[k]
    p, q, xk = th[r], th[ci], x[k]
    e = xk - (p * q).sum(1)
    ee = (c.dpad + 2) * U24 * np.abs(p * q).sum(1) + U24 * np.abs(e)
    ww = np.where(xk > 0, f32(c.w), 0.0)
    return SimpleNamespace(k=k, bpos=bpos, r=r, ci=ci, p=p, q=q, x=xk, e=e, ee=ee, ww=ww)


def _scatter(c, en, tP, eP, tQ, eQ, flaw):
    """Row sums of the per-entry terms: P rows get tP (summed in 256 / dpad strided parts), Q rows tQ (in batch order).
    Returns (sum, bound) of shape [(R + I), dpad]."""
    n = c.R + c.I
    s, a, E, cnt = np.zeros((n, c.dpad)), np.zeros((n, c.dpad)), np.zeros((n, c.dpad)), np.zeros(n)
    keep = en.bpos < c.dpad if flaw == "first_block_only" else np.ones(len(en.k), dtype=bool)
    for idx, t, e, kp in ((en.r, tP, eP, np.ones(len(en.k), dtype=bool)), (en.ci, tQ, eQ, keep)):
        np.add.at(s, idx[kp], t[kp])
        np.add.at(a, idx[kp], np.abs(t[kp]))
        np.add.at(E, idx[kp], e[kp])
        np.add.at(cnt, idx[kp], 1)
    cnt[: c.R] += 256 // c.dpad
    return s, (cnt[:, None] + 2) * U24 * a + E


def batch_grad(c, th, rows, flaw=None):
    """d/d theta of sum w [X > 0] (X - p . q)^2 over the batch's stored entries, its bound, and the entries."""
    en = _batch_entries(c, th, rows)
    we = (en.ww * en.e)[:, None]
    tP, tQ = we * en.q, we * en.p
    eP = (en.ww * en.ee)[:, None] * np.abs(en.q) + 2 * U24 * np.abs(tP)
    eQ = (en.ww * en.ee)[:, None] * np.abs(en.p) + 2 * U24 * np.abs(tQ)
    s, se = _scatter(c, en, tP, eP, tQ, eQ, flaw)
    f = -4.0 if flaw == "factor2" else -2.0
    return f * s, 2.0 * se, en


def _grad(c, th, rows, flaw):
    bp, bpe, en = batch_grad(c, th, rows, flaw)
    wd = f32(c.wd)
    g = bp + wd * th
    return g, bpe + U24 * np.abs(wd * th) + U24 * np.abs(g), en


def step_ref(c, theta, m, v, perm, j, adam_t, flaw=None):
    """Step j of an epoch (rk_aia_forward): the gradient over the batch's stored entries plus wd theta, then torch-order Adam
    with step_size and bc2s rounded to fp32 from double.  Returns (theta', m', v'), (bounds of the three)."""
    th, m, v = _state(c, theta), _state(c, m), _state(c, v)
    g, ge, _ = _grad(c, th, batch_rows(c, perm, j), flaw)
    return adam_ref(th, m, v, g, ge, c.lr, c.b1, c.b2, c.eps, adam_t)


def reverse_ref(c, theta, m1, v1, adj_th, adj_m, adj_v, perm, j, adam_t, flaw=None):
    """The adjoint of step j (rk_aia_reverse with hi = lo + 1) from theta of slot k, m' and v' of slot k + 1 and the incoming
    adjoints of theta', m', v'.  Where v' == 0 the 1 / sqrt(v') term of v-bar is 0 (include/recad_hip.h).
    Returns a dict of (value, bound) pairs: gbar, adj_th, adj_m, adj_v [(R + I), dpad] and xbar [n_fake_nz], the increment."""
    th, mo, vo = _state(c, theta), _state(c, m1), _state(c, v1)
    thb, mb, vb = _state(c, adj_th), _state(c, adj_m), _state(c, adj_v)
    w1, b2, w2, step, bc2s, eps = adam_consts(c.lr, c.b1, c.b2, c.eps, adam_t)
    b1, wd = f32(c.b1), f32(c.wd)
    rows = batch_rows(c, perm, j)
    g, ge, en = _grad(c, th, rows, flaw)
    # ---- the element-wise adjoint of Adam: 3 roundings in D, 5 in a, 14 in ct
    sv = np.sqrt(vo)
    D = sv / bc2s + eps
    a = step * thb / D
    mh = mb - a
    mhe = 5 * U24 * np.abs(a) + U24 * np.abs(mh)
    pos = vo > 0
    ct = np.where(pos, step * thb * mo / (2 * bc2s * D * D * np.where(pos, sv, 1.0)), 0.0)
    vh = vb + ct
    vhe = 14 * U24 * np.abs(ct) + U24 * np.abs(vh)
    t2 = 2 * w2 * g * vh
    gb = w1 * mh + t2
    gbe = w1 * mhe + 2 * w2 * (np.abs(vh) * ge + np.abs(g) * vhe) + U24 * np.abs(w1 * mh) + 4 * U24 * np.abs(t2) + U24 * np.abs(gb)
    am, av = b1 * mh, b2 * vh
    ame, ave = b1 * mhe + U24 * np.abs(am), b2 * vhe + U24 * np.abs(av)
    # ---- the batch part: theta-bar += (d g / d theta)^T gbar, X-bar += (d g / d X)^T gbar
    gp, gq, gpe, gqe = gb[en.r], gb[en.ci], gbe[en.r], gbe[en.ci]
    p, q, e, ee, ww = en.p, en.q, en.e[:, None], en.ee[:, None], en.ww[:, None]
    s = (gp * q + gq * p).sum(1)[:, None]
    se = ((np.abs(q) * gpe + np.abs(p) * gqe).sum(1) + (2 * c.dpad + 2) * U24 * (np.abs(gp * q) + np.abs(gq * p)).sum(1))[:, None]
    tP, tQ = ww * (s * q - e * gq), ww * (s * p - e * gp)
    eP = ww * (np.abs(q) * se + np.abs(gq) * ee + np.abs(e) * gqe) + 3 * U24 * ww * (np.abs(s * q) + np.abs(e * gq))
    eQ = ww * (np.abs(p) * se + np.abs(gp) * ee + np.abs(e) * gpe) + 3 * U24 * ww * (np.abs(s * p) + np.abs(e * gp))
    acc, acce = _scatter(c, en, tP, eP, tQ, eQ, flaw)
    f = 4.0 if flaw == "factor2" else 2.0
    wt = np.zeros_like(gb) if flaw == "no_wd_gbar" else wd * gb
    ath = thb + wt + f * acc
    athe = wd * gbe + 2 * acce + 3 * U24 * (np.abs(thb) + np.abs(wt) + np.abs(f * acc))
    fake = en.k >= c.nnz_real
    xb, xbe = np.zeros(c.n_fake_nz), np.zeros(c.n_fake_nz)
    wx = np.ones_like(ww) if flaw == "xbar_no_w" else ww
    xb[en.k[fake] - c.nnz_real] = (-f * wx * s)[fake, 0]
    xbe[en.k[fake] - c.nnz_real] = (2 * ww * se)[fake, 0] + 2 * U24 * np.abs(xb[en.k[fake] - c.nnz_real])
    return {"gbar": (gb, gbe), "adj_th": (ath, athe), "adj_m": (am, ame), "adj_v": (av, ave), "xbar": (xb, xbe)}


# ---------------------------------------------------------------- attack loss
def attack_loss_ref(c, theta, tgt, pair_ptr, pair_user, pair_tgt, pair_slot, tscale, wide=False, flaw=None, near_ok=False):
    """G_loss = sum_t mean_u(-log_softmax(z_u)[t] / 1.1) / 10 with z_ui = s_ui [i == t or s_ui >= s_ut], and its gradient at
    theta.  Returns (loss, bound), (adj, bound) with adj [(R + I), dpad]: P-bar on the real users' rows, 0 on the fake rows,
    Q-bar on the item rows.  wide: the overflow case (K_EXP_WIDE, arguments down to EXP_WIDE_LO).  near_ok: do not refuse near
    ties (for a caller that compares under a tolerance of its own and not under the bounds)."""
    th = _state(c, theta)
    K, lo = (K_EXP_WIDE, EXP_WIDE_LO) if wide else (K_ULP, -20.0)
    KU = K * 2.0 ** -23
    I, DP = c.I, c.dpad
    Q = th[c.R:]
    pair_user, t, slot = (np.asarray(a, dtype=np.int64) for a in (pair_user, pair_tgt, pair_slot))
    n_p = len(pair_user)
    assert n_p and pair_user.max() < c.n_real
    pu = th[pair_user]
    S, A = np.zeros((n_p, I)), np.zeros((n_p, I))
    for d in range(DP):                       # one elementwise pass per column: equal Q rows give equal bits
        S += pu[:, d, None] * Q[None, :, d]
        A += np.abs(pu[:, d, None] * Q[None, :, d])
    es = (DP + 2) * U24 * A
    ar = np.arange(n_p)
    st, est = S[ar, t], es[ar, t]
    is_t = np.arange(I)[None, :] == t[:, None]
    near = ~is_t & (S != st[:, None]) & (np.abs(S - st[:, None]) <= es + est[:, None])
    assert near_ok or not near.any(), "a score within rounding of its target's: the masked loss has no bound there"
    M = is_t | ((S > st[:, None]) if flaw == "strict_tie" else (S >= st[:, None]))
    z, ez = np.where(M, S, 0.0), np.where(M, es, 0.0)
    mx = z.max(1)
    ex = np.exp(z - mx[:, None])
    sm = ex.sum(1)
    l = mx + np.log(sm)
    soft = ex / sm[:, None]
    arg = np.where(M, S - l[:, None], 0.0)
    assert (z - mx[:, None]).min() >= lo and arg.min() >= lo and arg.max() <= 20.0, "an expf argument outside the measured range"
    stages = math.ceil(I / 64) + 7           # rescalings a term can go through: the lane's loop and the six butterfly steps
    rel_sm = stages * (KU + (np.abs(z - mx[:, None]).max(1) + 2) * U24) + I * KU * FLT_MIN
    le = (soft * ez).sum(1) + rel_sm + KU * np.abs(np.log(sm)) + U24 * (np.abs(l) + np.abs(mx))
    pl = -(st - l) / 1.1
    ple = (est + le + U24 * np.abs(st - l)) / 1.1 + 3 * U24 * np.abs(pl)
    means, me = [], 0.0
    for s_ in range(len(tgt)):
        b, e = int(pair_ptr[s_]), int(pair_ptr[s_ + 1])
        n = e - b
        means.append(pl[b:e].sum() / n)
        me += (ple[b:e].sum() + (math.ceil(n / 64) + 8) * U24 * np.abs(pl[b:e]).sum()) / n + U24 * abs(means[-1])
    loss = sum(means) / 10.0
    loss_err = (me + (len(tgt) + 1) * U24 * sum(abs(x) for x in means)) / 10.0 + U24 * abs(loss)
    # ---- gradient: dF / ds_ui = (M softmax_i - [i == t]) tscale[slot]
    sc = np.asarray(tscale, dtype=np.float64)[slot][:, None]
    soft_l = np.where(M, np.exp(arg), 0.0)
    g = soft_l - is_t
    arge = es + le[:, None] + U24 * np.abs(S - l[:, None])
    ge = np.where(M, soft_l * (arge + KU) + KU * FLT_MIN, 0.0)
    gs = g * sc
    gse = sc * (ge + U24 * np.abs(g)) + U24 * np.abs(gs)
    adj, adje = np.zeros_like(th), np.zeros_like(th)
    aq = np.abs(Q)
    cP, aP, eP = gs @ Q, np.abs(gs) @ aq, gse @ aq
    sP, saP, seP, cnt = np.zeros((c.R, DP)), np.zeros((c.R, DP)), np.zeros((c.R, DP)), np.zeros(c.R)
    np.add.at(sP, pair_user, cP)
    np.add.at(saP, pair_user, aP)
    np.add.at(seP, pair_user, eP)
    np.add.at(cnt, pair_user, 1)
    adj[: c.R] = sP
    adje[: c.R] = (cnt[:, None] * math.ceil(I / 64) + 8) * U24 * saP + seP
    adj[c.R:] = gs.T @ pu
    adje[c.R:] = (math.ceil(n_p / 64) + 8) * U24 * (np.abs(gs).T @ np.abs(pu)) + gse.T @ np.abs(pu)
    return (loss, loss_err), (adj, adje)


# ---------------------------------------------------------------- project and the G step
def project_ref(gen):
    """clamp(round_half_even(gen), 0, 5), exactly (fp32 in, fp32 out)."""
    return np.clip(np.rint(np.asarray(gen, dtype=np.float32)), np.float32(0), np.float32(5)).astype(np.float32)


def g_step_ref(p, m, v, g, lr, b1, b2, eps, t):
    """rk_aia_g_step: adam_ref on an exact gradient, no weight decay."""
    f = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    return adam_ref(f(p), f(m), f(v), f(g), 0.0, lr, b1, b2, eps, t)


def g_case(n, t):
    """Parameters, moments (zero at adam_t 1, warm otherwise) and three gradients for rk_aia_g_step."""
    rng = _rng(f"g{n}_{t}")
    p = rng.normal(0, 1, n).astype(np.float32)
    m = np.zeros(n, dtype=np.float32) if t == 1 else rng.normal(0, 0.3, n).astype(np.float32)
    v = np.zeros(n, dtype=np.float32) if t == 1 else rng.uniform(0.05, 0.5, n).astype(np.float32)
    return p, m, v, [rng.normal(0, 1, n).astype(np.float32) for _ in range(3)]


# ---------------------------------------------------------------- crafted cases shared by the CPU checks and the GPU tests
_DEF = dict(n_real=80, n_fake=20, F=5, I=50, w=1.0, wd=1e-5, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, adam_t=7, j=1, vzero=False)
WMF_CASES = {
    # name: d (dpad follows), batch, then what differs from _DEF.  c0 passes of the item-tile loop = ceil(nb / dpad).
    "d16_b40": dict(d=16, batch=40),                                          # 3 passes: 16, 16, 8
    "d1_b16": dict(d=1, batch=16, w=0.25, wd=0.0),                            # 1 pass, a full one
    "d20_b33": dict(d=20, batch=33, w=3.0, wd=0.1),                           # 2 passes: 32, 1
    "d32_b32": dict(d=32, batch=32),                                          # 1 pass
    "d64_b70": dict(d=64, batch=70, n_real=150, w=0.25, wd=0.1),              # 2 passes: 64, 6
    "d40_b40": dict(d=40, batch=40, w=3.0, wd=0.0),                           # 1 pass
    "d16_b256": dict(d=16, batch=256, n_real=500, n_fake=30, I=120, wd=0.1),  # 16 passes
    "last_one": dict(d=16, batch=40, n_real=61, j=2),                         # R = 81: the last batch is one row
    "all_R": dict(d=20, batch=64, n_real=40, n_fake=10, j=0, w=0.25),         # nb = R = 50
    "betas": dict(d=16, batch=40, lr=3e-3, b1=0.8, b2=0.99, eps=1e-6, adam_t=500, wd=0.1, w=3.0),
    "vzero": dict(d=16, batch=40, wd=0.0, vzero=True),
}


def wmf_case(name):
    """A crafted CSR, permutation, warm state (m, v with v' bounded away from 0: the 1 / (D^2 sqrt(v')) factor of v-bar would
    otherwise swamp any bound), incoming adjoints and X-bar prefill for step j of WMF_CASES[name].  Planted: the batch rows at
    positions 0 and nb - 1 both rate item 0 (different c0 blocks when nb > dpad); item I - 1 is rated by no batch row; with
    nb >= 6 a real batch row is empty and another stores a rating of 0; a fake batch row holds a projection of 0."""
    k = dict(_DEF, **WMF_CASES[name])
    rng = _rng(name)
    n_real, n_fake, F, I, d, batch, j = k["n_real"], k["n_fake"], k["F"], k["I"], k["d"], k["batch"], k["j"]
    R, dp = n_real + n_fake, dpad_of(k["d"])
    s0 = j * batch
    nb = min(batch, R - s0)
    assert nb >= 1
    n_fb = min(n_fake, max(1, nb // 4))
    fk, rl = n_real + rng.permutation(n_fake), rng.permutation(n_real)
    inb = rng.permutation(np.concatenate([fk[:n_fb], rl[: nb - n_fb]]))
    rest = rng.permutation(np.concatenate([fk[n_fb:], rl[nb - n_fb:]]))
    perm = np.concatenate([rest[:s0], inb, rest[s0:]]).astype(np.int32)
    assert len(perm) == R and np.array_equal(np.sort(perm), np.arange(R))
    invperm = np.argsort(perm).astype(np.int32)
    cols, vals = [], []
    for r in range(R):
        n = F if r >= n_real else int(rng.integers(2, 9))
        cols.append(np.sort(rng.choice(np.arange(1, I - 1), n, replace=False)))
        vals.append(rng.integers(1, 6, n).astype(np.float32))
    for r in {int(inb[0]), int(inb[-1])}:
        cols[r][0] = 0
    mid_real = [int(r) for r in inb[1:-1] if r < n_real]
    facts = dict(nb=nb, passes=math.ceil(nb / dp), empty=None, zero_rating=None, zero_fake=None)
    if nb >= 6:
        assert len(mid_real) >= 2
        cols[mid_real[0]], vals[mid_real[0]] = cols[mid_real[0]][:0], vals[mid_real[0]][:0]
        vals[mid_real[1]][-1] = 0
        facts.update(empty=mid_real[0], zero_rating=mid_real[1])
    fb = [int(r) for r in inb if r >= n_real]
    vals[fb[0]][-1] = 0
    facts["zero_fake"] = fb[0]
    out_real = [int(r) for r in rest if r < n_real]
    if out_real:
        cols[out_real[0]][-1] = I - 1
    rowptr = np.zeros(R + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(a) for a in cols])
    col, x = np.concatenate(cols).astype(np.int32), np.concatenate(vals).astype(np.float32)
    c = SimpleNamespace(R=R, n_real=n_real, I=I, d=d, dpad=dp, batch=batch, rowptr=rowptr, col=col, x=x, nnz_real=int(rowptr[n_real]),
                        n_fake_nz=int(rowptr[R] - rowptr[n_real]), lr=k["lr"], b1=k["b1"], b2=k["b2"], eps=k["eps"], wd=k["wd"], w=k["w"])
    n = R + I

    def pad(a):
        out = np.zeros((n, dp), dtype=np.float32)
        out[:, :d] = a
        return out

    theta, m = pad(rng.normal(0, 0.1, (n, d))), pad(rng.normal(0, 0.3, (n, d)))
    v = pad(rng.uniform(0.05, 0.5, (n, d)))
    adj = [pad(rng.normal(0, s, (n, d))) for s in (1.0, 0.3, 0.3)]
    if k["vzero"]:
        # a row in no batch with zero m and v (and wd = 0): m' = v' = 0, so D = eps and its m-hat is m-bar - (step / eps) theta-bar.
        # Its incoming theta-bar is scaled by eps / lr so that m-hat stays of the size of the other rows' and the row sits under
        # the same cap as the rest of its tensor
        facts["vzero_row"] = out_real[1]
        m[out_real[1]] = 0
        v[out_real[1]] = 0
        adj[0][out_real[1]] *= np.float32(k["eps"] / k["lr"])
    xbar0 = rng.normal(0, 1.0, c.n_fake_nz).astype(np.float32)
    return SimpleNamespace(name=name, c=c, perm=perm, invperm=invperm, j=j, adam_t=k["adam_t"], theta=theta, m=m, v=v, adj=adj, xbar0=xbar0,
                           rows=inb.astype(np.int64), facts=facts)


def wmf_facts(case):
    """What the case's input really holds, for the tests to assert: the planted edges and the cross-block item."""
    c, rows, f = case.c, case.rows, dict(case.facts)
    ptr, col, x = c.rowptr, c.col, c.x
    blocks = {}
    for pos, r in enumerate(rows):
        for kk in range(ptr[r], ptr[r + 1]):
            if x[kk] > 0:
                blocks.setdefault(int(col[kk]), set()).add(pos // c.dpad)
    f["cross_block"] = any(len(b) > 1 for b in blocks.values())
    rated = set(int(col[kk]) for r in rows for kk in range(ptr[r], ptr[r + 1]))
    f["unrated_item"] = (c.I - 1) not in rated
    f["empty_ok"] = f["empty"] is not None and ptr[f["empty"]] == ptr[f["empty"] + 1] and f["empty"] in rows
    zr = f["zero_rating"]
    f["zero_rating_ok"] = zr is not None and zr in rows and zr < c.n_real and bool((x[ptr[zr]:ptr[zr + 1]] == 0).any())
    zf = f["zero_fake"]
    f["zero_fake_ok"] = zf in rows and zf >= c.n_real and bool((x[ptr[zf]:ptr[zf + 1]] == 0).any())
    # rk_find_sorted lands on the first and on the last entry of a row: a batch row of three or more entries whose two end entries are
    # weighed (X > 0) at columns that exist -- the groups of those two items search this row and must find exactly these entries
    f["first_last"] = any(ptr[r + 1] - ptr[r] >= 3 and x[ptr[r]] > 0 and x[ptr[r + 1] - 1] > 0
                          and 0 <= col[ptr[r]] < col[ptr[r + 1] - 1] < c.I for r in rows)
    f["has_fake"] = any(r >= c.n_real for r in rows)
    return f


LOSS_CASES = {
    # name: I, U (real users), d, targets, ties (items that copy the first target's Q row), scale of theta, wide
    "i37_u5": dict(I=37, U=5, d=16, n_tgt=1),
    "i64_u6": dict(I=64, U=6, d=20, n_tgt=2),
    "i65_u7": dict(I=65, U=7, d=64, n_tgt=3),
    "i130_u130": dict(I=130, U=130, d=10, n_tgt=2),
    "ties": dict(I=65, U=7, d=16, n_tgt=2, ties=2),
    "overflow": dict(I=37, U=5, d=16, n_tgt=1, scale=3.0, wide=True),
}


def loss_case(name):
    """theta and the (user, target) pairs of one attack-loss call.  The pair count of every target and the total are not
    multiples of 4; with two or more targets user 0 is a pair of the first two and user 1 of none."""
    k = dict(dict(ties=0, scale=0.3, wide=False, n_fake=3), **LOSS_CASES[name])
    rng = _rng(name)
    I, U, d, n_tgt = k["I"], k["U"], k["d"], k["n_tgt"]
    R, dp = U + k["n_fake"], dpad_of(d)
    theta = np.zeros((R + I, dp), dtype=np.float32)
    theta[:, :d] = rng.normal(0, k["scale"], (R + I, d))
    tgt = np.sort(rng.choice(I - 1, n_tgt, replace=False)).astype(np.int32)
    tgt[-1] = I - 1 if n_tgt > 1 else tgt[-1]                     # the last item is a target too
    dup = np.setdiff1d(np.arange(I), tgt)[: k["ties"]] if k["ties"] else np.zeros(0, dtype=np.int64)
    theta[R + dup] = theta[R + tgt[0]]
    users, ptr, slots, tg = [], [0], [], []
    pidx = np.full((n_tgt, U), -1, dtype=np.int32)
    for s, t in enumerate(tgt):
        pool = np.arange(2, U) if n_tgt > 1 else np.arange(U)
        n = int(rng.integers(1, len(pool) + 1))
        us = np.sort(rng.choice(pool, n, replace=False))
        if n_tgt > 1 and s < 2:
            us = np.concatenate([[0], us])
        while len(us) % 4 == 0 or (s == n_tgt - 1 and (len(users) + len(us)) % 4 == 0):
            us = us[:-1]
        pidx[s, us] = len(users) + np.arange(len(us))
        users.extend(int(u) for u in us)
        slots.extend([s] * len(us))
        tg.extend([int(t)] * len(us))
        ptr.append(len(users))
    c = SimpleNamespace(R=R, n_real=U, I=I, d=d, dpad=dp, batch=16, nnz_real=0, n_fake_nz=0, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, w=1.0)
    i32 = lambda a: np.asarray(a, dtype=np.int32)      # noqa: E731
    tscale = np.asarray([1.0 / (11.0 * (ptr[s + 1] - ptr[s])) for s in range(n_tgt)], dtype=np.float32)
    return SimpleNamespace(name=name, c=c, theta=theta, tgt=tgt, pair_ptr=i32(ptr), pair_user=i32(users), pair_tgt=i32(tg), pair_slot=i32(slots),
                           pidx=pidx, tscale=tscale, dup=dup, wide=k["wide"])


def loss_args(case):
    return (case.c, case.theta, case.tgt, case.pair_ptr, case.pair_user, case.pair_tgt, case.pair_slot, case.tscale)
