"""float64 numpy restatement of the AUSH attacker's device operations (csrc/aush.hip), for the tests: the counter-based
draws in Python integers, the sampler, the ZR rule, the generator at S, and one discriminator step -- the four losses, the
gradient of every parameter and a first-order running bound on the error of the fp32 kernels beside each value.  It is
written from the formulas (aush.py:60-167 of the reference); nothing here is the product's code path, and
tests/test_attacker_host.py checks it against torch autograd and the reference's recorded losses.

Error bounds.  u = 2^-24 is fp32's unit roundoff.  A sequential fp32 dot product of n terms (fused or not) is within
(n + 2) u sum |a_i b_i| of the exact one; the device sigmoid 1 / (1 + expf(-z)) is within
0.25 err(z) + s ((1 - s) K 2^-23 + 2^-23) of sigma(z), K = the ulp error of expf (one rounding each for the add and the
division); logf / log1pf are within K 2^-23 |result|.  The bounds are carried through the three layers forward and
backward.  Backward, everything of one row is linear in that row's dz4, so dz4's relative error is carried as one factor per
row (it multiplies dz3, dz2 and dz1 of the row alike) and only the remaining, independent errors go through the absolute
sums.  All of it is first order: products of two errors are dropped."""
import math

import numpy as np

HG, HD = 128, 150
SENTINEL = 0x7FFFFFFF
U24, U52 = 2.0 ** -24, 2.0 ** -52
TAIL = ("main.0.bias", "main.2.weight", "main.2.bias", "main.4.weight", "main.4.bias", "main.6.weight", "main.6.bias")
M64 = (1 << 64) - 1
# Weight scale of the crafted discriminators (times torch's Linear range): with the full range the bound on the b1 and W1
# gradients passes its cap of 2^-10 of the tensor's largest entry only barely or not at all; at half the range every one does.
CRAFT_W = 0.5
# Largest error of the device's expf / logf / log1pf in ulps of the result.  The ROCm installation carries no accuracy table
# for its device library, so it was measured once on an MI355X against fp64 (2^22 arguments, half on a grid, half random:
# expf on [-20, 20]; logf(x) and log1pf(-x) at x = the fp32 sigmoid of those arguments, the only way the kernels call them):
# expf 0.84, logf 2.14, log1pf 0.56.  K_ULP is twice the largest; it is the only measured margin of the AUSH kernel tests.
K_ULP = 2 * 2.15


# ---------------------------------------------------------------- the draws, in Python integers (common.h, aush.hip:27)
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_key(seed, stream, row, draw):
    return mix64(seed ^ mix64(stream ^ mix64(((row << 20) & M64) ^ draw)))


def pool_pick(seed, stream, row, k, pool_col, pb, deg):
    """Draw k of row `row`: a pool entry by the high-word multiply, or the sentinel for an empty pool."""
    if deg <= 0:
        return SENTINEL
    x = draw_key(seed, stream, row, k)
    return int(pool_col[pb + (((x >> 32) * deg) >> 32)])


def perm_order(n, seed, stream):
    """Positions of rk_aush_permute's output: a stable sort of the keys draw_key(seed, stream, i, 0x7ffff)."""
    keys = [draw_key(seed, stream, i, 0x7FFFF) for i in range(n)]
    return np.asarray(sorted(range(n), key=lambda i: (keys[i], i)), dtype=np.int64)


def zr_mask(sval, batch, zr_ratio, seed, stream):
    """rk_aush_zr: per batch, of the n pairs with sval == 0 the n - floor(n (1 - ratio)) of smallest key (ties: position)."""
    sval = np.asarray(sval)
    N, S = sval.shape
    out = np.zeros((N, S), dtype=np.uint8)
    for r0 in range(0, N, batch):
        rows = min(batch, N - r0)
        keyed = []
        for p in range(rows * S):
            if sval[r0 + p // S, p % S] == 0:
                keyed.append((draw_key(seed, stream ^ 0x5A5A5A5A, r0 + p // S, 0x40000 + p % S) | 1, p))
        n = len(keyed)
        n_keep = n - int(math.floor(float(n) * (1.0 - float(zr_ratio))))
        for _, p in sorted(keyed)[:n_keep]:
            out[r0 + p // S, p % S] = 1
    return out


def eligible_ref(ptr, idx, val, excl, F):
    """(pool_ptr, pool_col, eligible) of rk_aush_eligible."""
    pool, el, pp = [], [], [0]
    for u in range(len(ptr) - 1):
        c, v = idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]]
        keep = c[(v > 0) & ~np.isin(c, excl)]
        pool.append(keep)
        pp.append(pp[-1] + len(keep))
        if len(keep) >= F:
            el.append(u)
    col = np.concatenate(pool) if pool and pp[-1] else np.zeros(0, dtype=np.int32)
    return np.asarray(pp, dtype=np.int32), col.astype(np.int32), np.asarray(el, dtype=np.int32)


def _rating(c, v, item):
    p = int(np.searchsorted(c, item))
    return v[p] if p < len(c) and c[p] == item else np.float32(0)


def sample_ref(ptr, idx, val, users, draws, sel):
    """rk_aush_sample on given draws [n, F] (the sentinel = no draw): fcol / fval padded with (sentinel, 0), nf, sval."""
    draws = np.asarray(draws, dtype=np.int64)
    n, F = draws.shape
    fcol = np.full((n, F), SENTINEL, dtype=np.int32)
    fval = np.zeros((n, F), dtype=np.float32)
    nf = np.zeros(n, dtype=np.int32)
    sval = np.zeros((n, len(sel)), dtype=np.float32)
    for r, u in enumerate(users):
        c, v = idx[ptr[u]:ptr[u + 1]], val[ptr[u]:ptr[u + 1]]
        d = np.unique(draws[r][draws[r] != SENTINEL])
        nf[r] = len(d)
        fcol[r, :len(d)] = d
        fval[r, :len(d)] = [_rating(c, v, x) for x in d]
        sval[r] = [_rating(c, v, s) for s in sel]
    return fcol, fval, nf, sval


def own_draws(users, F, pool_ptr, pool_col, seed, stream, row0):
    """The draws rk_aush_sample makes itself (draws == NULL)."""
    out = np.empty((len(users), F), dtype=np.int64)
    for r, u in enumerate(users):
        pb, deg = int(pool_ptr[u]), int(pool_ptr[u + 1] - pool_ptr[u])
        out[r] = [pool_pick(seed, stream, row0 + r, k, pool_col, pb, deg) for k in range(F)]
    return out


# ---------------------------------------------------------------- generator and discriminator
def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _sig_err(s, ez, K):
    return 0.25 * ez + s * ((1.0 - s) * K * 2.0 ** -23 + 2.0 ** -23)


def pack_d(D):
    """The reference's discriminator state (torch layout) as the device's packed buffer, float64."""
    D = {k: np.asarray(v, dtype=np.float64) for k, v in D.items()}
    return np.concatenate([D["main.0.weight"].T.reshape(-1)] + [D[k].reshape(-1) for k in TAIL])


def unpack_d(p, I):
    """Views of a packed buffer: W1t [I, 150] and the seven tail tensors in torch shapes."""
    p = np.asarray(p)
    shapes = {"main.0.bias": (HD,), "main.2.weight": (HD, HD), "main.2.bias": (HD,), "main.4.weight": (HD, HD),
              "main.4.bias": (HD,), "main.6.weight": (1, HD), "main.6.bias": (1,)}
    out, o = {"W1t": p[: I * HD].reshape(I, HD)}, I * HD
    for k in TAIL:
        n = int(np.prod(shapes[k]))
        out[k] = p[o:o + n].reshape(shapes[k])
        o += n
    assert o == len(p)
    return out


def gen_ref(fcol, fval, nf, w1t, b1, w2, b2, sel, K=0.0):
    """rk_aush_gen in fp64 and the bound on the fp32 kernel's error: (gen [n, S], bound [n, S])."""
    w1t, b1, w2, b2 = (np.asarray(a, dtype=np.float64) for a in (w1t, b1, w2, b2))
    fcol, fval, nf = np.asarray(fcol), np.asarray(fval, dtype=np.float64), np.asarray(nf)
    live = np.arange(fcol.shape[1])[None, :] < nf[:, None]
    Wg = w1t[np.where(live, fcol, 0)] * live[..., None]
    x = fval * live
    z1 = np.einsum("rk,rkj->rj", x, Wg) + b1
    e1 = (nf[:, None] + 2) * U24 * (np.einsum("rk,rkj->rj", np.abs(x), np.abs(Wg)) + np.abs(b1))
    h = _sig(z1)
    eh = _sig_err(h, e1, K)
    z2 = h @ w2[sel].T + b2[sel]
    e2 = (HG + 2) * U24 * (h @ np.abs(w2[sel]).T + np.abs(b2[sel])) + eh @ np.abs(w2[sel]).T
    s = _sig(z2)
    return 5.0 * s, 5.0 * _sig_err(s, e2, K) + U24 * 5.0 * s


def _entries(fcol, fval, nf, sval, gen, sel):
    """The D input of each row as the kernel forms it: columns [B, F + S] (sentinel = padding), real and fake values."""
    fcol, nf, sel = np.asarray(fcol), np.asarray(nf), np.asarray(sel)
    B, F = fcol.shape
    live = np.arange(F)[None, :] < nf[:, None]
    ec = np.concatenate([np.where(live, fcol, SENTINEL), np.broadcast_to(sel, (B, len(sel)))], axis=1).astype(np.int64)
    fv = np.where(live, np.asarray(fval, dtype=np.float64), 0.0)
    gen = np.asarray(gen)
    # the kernel adds 5 in fp32; given fp32 values the same rounded sum is formed here, so it is no error of the kernel's
    vf = (gen + np.float32(5.0)).astype(np.float64) if gen.dtype == np.float32 else gen.astype(np.float64) + 5.0
    return ec, np.concatenate([fv, np.asarray(sval, dtype=np.float64)], axis=1), np.concatenate([fv, vf], axis=1)


def _forward(P, ec, ev, K):
    live = ec != SENTINEL
    Wg = P["W1t"][np.where(live, ec, 0)] * live[..., None]
    W2, W3, w4 = P["main.2.weight"], P["main.4.weight"], P["main.6.weight"][0]
    b1, b2, b3, b4 = P["main.0.bias"], P["main.2.bias"], P["main.4.bias"], P["main.6.bias"][0]
    z1 = np.einsum("rk,rkj->rj", ev, Wg) + b1
    e1 = (live.sum(1)[:, None] + 2) * U24 * (np.einsum("rk,rkj->rj", np.abs(ev), np.abs(Wg)) + np.abs(b1))
    h1 = _sig(z1)
    eh1 = _sig_err(h1, e1, K)
    z2 = h1 @ W2.T + b2
    h2 = _sig(z2)
    eh2 = _sig_err(h2, (HD + 2) * U24 * (h1 @ np.abs(W2).T + np.abs(b2)) + eh1 @ np.abs(W2).T, K)
    z3 = h2 @ W3.T + b3
    h3 = _sig(z3)
    eh3 = _sig_err(h3, (HD + 2) * U24 * (h2 @ np.abs(W3).T + np.abs(b3)) + eh2 @ np.abs(W3).T, K)
    z4 = h3 @ w4 + b4
    x = _sig(z4)
    ex = _sig_err(x, (HD + 2) * U24 * (h3 @ np.abs(w4) + abs(b4)) + eh3 @ np.abs(w4), K)
    return dict(h1=h1, h2=h2, h3=h3, z4=z4, x=x, eh1=eh1, eh2=eh2, eh3=eh3, ex=ex)


def _bce(x, ex, y, K):
    """torch BCELoss terms (each log clamped at -100) and the bound on the kernel's fp32 values."""
    with np.errstate(divide="ignore"):
        l = -np.maximum(np.log(x), -100.0) if y == 1 else -np.maximum(np.log1p(-x), -100.0)
    return l, ex / np.maximum(x if y == 1 else 1.0 - x, 1e-300) + (K * 2.0 ** -23 + U24) * np.abs(l)


def _mean_err(l, el):
    """fp64 sum of B fp32 terms, divided by B, rounded to fp32."""
    return el.mean() + (len(l) * U52 + U24) * abs(l.mean())


def gan_loss(Pd, I, fcol, fval, nf, sval, gen, sel, K=0.0):
    """g_loss_gan = mean BCE(D(fake), 1) under the packed discriminator Pd, and its bound."""
    ec, _, ev_f = _entries(fcol, fval, nf, sval, gen, sel)
    f = _forward(unpack_d(np.asarray(Pd, dtype=np.float64), I), ec, ev_f, K)
    l, el = _bce(f["x"], f["ex"], 1, K)
    return l.mean(), _mean_err(l, el)


def d_step_ref(Pd, I, fcol, fval, nf, sval, gen, zr, sel, K=0.0):
    """One discriminator batch in fp64 at the packed parameters Pd [I * 150 + tail].

    Returns a dict: losses [4] (d_loss, g_loss_rec, g_loss_shilling, g_loss_gan at the same D) and loss_err [4]; gen is the
    caller's; grad / grad_err: the seven tail gradients in torch shapes; items (ascending), gw1 / gw1_err [n_items, 150]: the
    first-layer gradient of each item of the batch; g / g_err: all of it packed like Pd (zero off the batch's rows); and the
    per-row intermediates (dz1..dz4, h1..h3, ec, ev_r, ev_f) from which a test can take single contributions."""
    P = unpack_d(np.asarray(Pd, dtype=np.float64), I)
    ec, ev_r, ev_f = _entries(fcol, fval, nf, sval, gen, sel)
    B, S = ec.shape[0], len(sel)
    f = _forward(P, np.concatenate([ec, ec]), np.concatenate([ev_r, ev_f]), K)
    x, ex, h1, h2, h3 = f["x"], f["ex"], f["h1"], f["h2"], f["h3"]
    lr_, elr = _bce(x[:B], ex[:B], 1, K)
    lf_, elf = _bce(x[B:], ex[B:], 0, K)
    lg_, elg = _bce(x[B:], ex[B:], 1, K)
    d_loss = 0.5 * (lr_.mean() + lf_.mean())
    vf = ev_f[:, -S:]
    zr = np.asarray(zr).reshape(B, S).astype(np.float64)
    gen64 = np.asarray(gen, dtype=np.float64).reshape(B, S)
    rec, shill = (vf ** 2 * zr).sum() / (B * I), (gen64 ** 2).sum() / (B * I)
    losses = np.array([d_loss, rec, shill, lg_.mean()])
    loss_err = np.array([0.5 * (_mean_err(lr_, elr) + _mean_err(lf_, elf)) + 2 * U24 * abs(d_loss),
                         ((B * S + 2) * U52 + U24) * rec, ((B * S + 2) * U52 + U24) * shill, _mean_err(lg_, elg)])
    # backward.  dz4 = 0.5 (x - y) / B where x (1 - x) is above the kernel's 1e-12 clamp; below it the kernel's own formula
    y = np.concatenate([np.ones(B), np.zeros(B)])
    dz4 = 0.5 * (x - y) / np.maximum(x * (1 - x), 1e-12) / B * (1 - x) * x
    rel = (0.5 / B * ex + 8 * U24 * np.abs(dz4)) / np.maximum(np.abs(dz4), 1e-300)     # one factor per row
    W2, W3, w4 = P["main.2.weight"], P["main.4.weight"], P["main.6.weight"][0]
    dz3 = dz4[:, None] * w4[None, :] * (1 - h3) * h3
    i3 = np.abs(dz4[:, None] * w4[None, :] * (1 - 2 * h3)) * f["eh3"] + 4 * U24 * np.abs(dz3)
    a2 = dz3 @ W3
    dz2 = a2 * (1 - h2) * h2
    i2 = (((HD + 2) * U24 * (np.abs(dz3) @ np.abs(W3)) + i3 @ np.abs(W3)) * (1 - h2) * h2 + np.abs(a2 * (1 - 2 * h2)) * f["eh2"]
          + 3 * U24 * np.abs(dz2))
    a1 = dz2 @ W2
    dz1 = a1 * (1 - h1) * h1
    i1 = (((HD + 2) * U24 * (np.abs(dz2) @ np.abs(W2)) + i2 @ np.abs(W2)) * (1 - h1) * h1 + np.abs(a1 * (1 - 2 * h1)) * f["eh1"]
          + 3 * U24 * np.abs(dz1))
    e4 = rel * np.abs(dz4)
    e3, e2, e1 = (rel[:, None] * np.abs(d) + i for d, i in ((dz3, i3), (dz2, i2), (dz1, i1)))
    R = 2 * B
    ru = (R + 2) * U24

    def outer(d, e, h, eh):
        return d.T @ h, ru * (np.abs(d).T @ np.abs(h)) + e.T @ np.abs(h) + np.abs(d).T @ eh

    grad, gerr = {}, {}
    grad["main.6.weight"], gerr["main.6.weight"] = outer(dz4[:, None], e4[:, None], h3, f["eh3"])
    grad["main.6.bias"], gerr["main.6.bias"] = np.array([dz4.sum()]), np.array([ru * np.abs(dz4).sum() + e4.sum()])
    grad["main.4.weight"], gerr["main.4.weight"] = outer(dz3, e3, h2, f["eh2"])
    grad["main.2.weight"], gerr["main.2.weight"] = outer(dz2, e2, h1, f["eh1"])
    for k, d, e in (("main.4.bias", dz3, e3), ("main.2.bias", dz2, e2), ("main.0.bias", dz1, e1)):
        grad[k], gerr[k] = d.sum(0), ru * np.abs(d).sum(0) + e.sum(0)
    # first layer: per item, its entries in (item, row) order, real then fake
    bb, kk = np.nonzero(ec != SENTINEL)
    items, inv = np.unique(ec[bb, kk], return_inverse=True)
    gw1, A, E = (np.zeros((len(items), HD)) for _ in range(3))
    for ev, rows in ((ev_r, bb), (ev_f, B + bb)):
        np.add.at(gw1, inv, ev[bb, kk][:, None] * dz1[rows])
        np.add.at(A, inv, np.abs(ev[bb, kk][:, None] * dz1[rows]))
        np.add.at(E, inv, np.abs(ev[bb, kk])[:, None] * e1[rows])
    cnt = np.bincount(inv, minlength=len(items))
    gw1_err = (2 * cnt[:, None] + 2) * U24 * A + E
    g, g_err = np.zeros(len(Pd)), np.zeros(len(Pd))
    gv, ev_ = unpack_d(g, I), unpack_d(g_err, I)
    gv["W1t"][items], ev_["W1t"][items] = gw1, gw1_err
    for k in TAIL:
        gv[k][...] = grad[k].reshape(gv[k].shape)
        ev_[k][...] = gerr[k].reshape(gv[k].shape)
    return dict(losses=losses, loss_err=loss_err, grad=grad, grad_err=gerr, items=items, gw1=gw1, gw1_err=gw1_err, g=g, g_err=g_err,
                dz1=dz1, dz2=dz2, dz3=dz3, dz4=dz4, h1=h1, h2=h2, h3=h3, x=x, z4=f["z4"], ec=ec, ev_r=ev_r, ev_f=ev_f)


def within(got, ref, bound):
    """The comparison of the GPU tests: every entry of got within its bound of ref (a NaN fails)."""
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound))


def capped(ref, bound):
    """A bound may not go vacuous: at most 2^-10 of the largest magnitude of the tensor it guards."""
    return bool(np.max(bound) <= 2.0 ** -10 * np.max(np.abs(ref)))


# ---------------------------------------------------------------- Adam (torch.optim.Adam, adam_elem of common.h)
def adam_consts(lr, b1, b2, eps, t):
    """The fp32 constants the device uses at step t, as float64: w1, b2, w2, step_size, bc2s, eps."""
    f = lambda a: float(np.float32(a))
    lr, b1, b2, eps = f(lr), f(b1), f(b2), f(eps)
    return f(1.0 - b1), b2, f(1.0 - b2), f(lr / (1.0 - b1 ** t)), f(math.sqrt(1.0 - b2 ** t)), eps


def adam_ref(p, m, v, g, g_err, lr, b1, b2, eps, t):
    """One adam_elem step in fp64 from the device's own fp32 state and constants, and the bound on each fp32 result given
    the bound g_err on the gradient: (p, m, v), (p_err, m_err, v_err)."""
    w1, b2, w2, step, bc2s, eps = adam_consts(lr, b1, b2, eps, t)
    m1 = m + w1 * (g - m)
    v1 = v * b2 + w2 * g * g
    den = np.sqrt(v1) / bc2s + eps
    upd = step * (m1 / den)
    em = w1 * g_err + 3 * U24 * (np.abs(m) + np.abs(g))
    ev = 2 * w2 * np.abs(g) * g_err + 4 * U24 * v1
    # |sqrt(a) - sqrt(b)| is at most both |a - b| / (2 sqrt(min)) (first order) and sqrt|a - b|
    eden = np.minimum(ev / np.maximum(2 * np.sqrt(v1), 1e-300), np.sqrt(ev)) / bc2s + 3 * U24 * den
    eu = step * (em / den + np.abs(m1) * eden / den ** 2) + 2 * U24 * np.abs(upd)
    return (p - upd, m1, v1), (eu + U24 * np.abs(p - upd), em, ev)


def adam_step64(D, m0, v0, grad, gw1, lr, t, I, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam in plain fp64 on the reference's state dict D (torch layout): the tail tensors from grad, the
    first-layer columns from gw1 {item: gradient}; a column whose moments are zero and that has no gradient does not move."""
    Dn = {k: v.astype(np.float64).copy() for k, v in D.items()}
    W1 = Dn["main.0.weight"]
    for k, gk in list(grad.items()) + [("w1", None)]:
        if k == "w1":
            touched = np.nonzero(np.any(m0["main.0.weight"] != 0, axis=0) | np.isin(np.arange(I), list(gw1)))[0]
            gfull = np.zeros((HD, len(touched)))
            for j, c in enumerate(touched):
                if int(c) in gw1:
                    gfull[:, j] = gw1[int(c)]
            m = b1 * m0["main.0.weight"][:, touched] + (1 - b1) * gfull
            v = b2 * v0["main.0.weight"][:, touched] + (1 - b2) * gfull ** 2
            W1[:, touched] -= lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
            continue
        m = b1 * m0[k] + (1 - b1) * gk
        v = b2 * v0[k] + (1 - b2) * gk ** 2
        Dn[k] = Dn[k] - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return Dn


# ---------------------------------------------------------------- one train batch from the rating CSR (aush.py:128-167)
def _restate_batch(D, G, ptr, idx, val, users, draws, zr, S, I, lr, t):
    """One discriminator step in float64 from the reference's formulas, on the users' CSR rows, their filler draws and ZR
    mask; returns (d_loss, gen, tail gradients, {item: first-layer gradient}, D -> D(fake) under another D)."""
    out = restate_batch_full(D, G, ptr, idx, val, users, draws, zr, S, I)
    rows, gen = out["rows"], out["gen"]

    def fake_fwd(Dp):
        ec, _, ev_f = _entries(*rows[:3], rows[3], gen, S)
        return _forward(unpack_d(pack_d(Dp), I), ec, ev_f, 0.0)["x"]

    grad = {k: out["grad"][k].reshape(np.asarray(D[k]).shape) for k in TAIL}
    return out["losses"][0], gen, grad, {int(c): out["gw1"][j] for j, c in enumerate(out["items"])}, fake_fwd


def restate_batch_full(D, G, ptr, idx, val, users, draws, zr, S, I, K=0.0):
    """d_step_ref (all four losses, every gradient) on the rows that the users, draws and ZR mask define, with the
    generator evaluated in fp64 (no fp32 rounding of gen anywhere); adds "rows" = (fcol, fval, nf, sval) and "gen"."""
    S = np.asarray(S, dtype=np.int64)
    rows = sample_ref(ptr, idx, val, users, draws, S)
    gen, _ = gen_ref(*rows[:3], np.asarray(G["main.0.weight"], dtype=np.float64).T, G["main.0.bias"], G["main.2.weight"],
                     G["main.2.bias"], S)
    out = d_step_ref(pack_d(D), I, *rows, gen, zr, S, K)
    out["rows"], out["gen"] = rows, gen
    return out


# ---------------------------------------------------------------- crafted inputs shared by the CPU power checks and the GPU tests
def craft_params(I, seed, w=1.0, b4=2.0):
    """A packed fp32 discriminator with torch's Linear ranges times w: uniform in +-w / sqrt(fan_in).  b4 is set apart from 0:
    with D(real) ~ D(fake) ~ 0.5 the real and the fake half of every gradient sum nearly cancel, and what is left is small
    beside the rounding of its terms; with x ~ sigma(b4) the two halves weigh (x - 1) and x."""
    rng = np.random.default_rng(seed)
    u = lambda n, fan: rng.uniform(-w / np.sqrt(fan), w / np.sqrt(fan), n)
    parts = [u(I * HD, I), u(HD, I), u(HD * HD, HD), u(HD, HD), u(HD * HD, HD), u(HD, HD), u(HD, HD), [b4]]
    return np.concatenate(parts).astype(np.float32)


def craft_rows(B, F, S, I, seed, shared=True, sel_last=True, sel=None):
    """Sampled rows of one batch as rk_aush_sample leaves them, built to hit the segment machinery's edges.

    sel_last: item I - 1 is selected (the largest id of the batch is an S item, its segment ends at the valid count) and item
    0 is a filler; otherwise item 0 is selected and I - 1 is a filler of row 0 only.  shared: one filler sits in every row (its
    segment is as long as an S item's) and every row has fillers; otherwise row 2 (the last row when B < 3) has none.  Row 0 also
    holds a filler no other row has, row 1 has nf < F.  Ratings 1..5 with a few 0 (a drawn item the user has not rated);
    sval is 0 for about half the pairs and zr marks a random part of those."""
    rng = np.random.default_rng(seed)
    rest = rng.choice(np.arange(1, I - 1), S - 1, replace=False)
    sel = np.sort(np.concatenate([rest, [I - 1 if sel_last else 0]])).astype(np.int32) if sel is None else np.asarray(sel, dtype=np.int32)
    low = int(np.setdiff1d(np.arange(1, 6), sel)[0])
    c_all, c_one = ((0, low) if shared else (low, 0)) if sel_last else (low, I - 1)
    pool = np.setdiff1d(np.arange(I), np.concatenate([sel, [c_all, c_one]]))
    fcol = np.full((B, F), SENTINEL, dtype=np.int32)
    fval = np.zeros((B, F), dtype=np.float32)
    nf = np.zeros(B, dtype=np.int32)
    empty = -1 if shared else min(2, B - 1)
    for r in range(B):
        n = 0 if r == empty else (F if r == 0 else (max(1, F // 2) if r == 1 else int(rng.integers(1, F + 1))))
        fixed = ([c_all] if shared else []) + ([c_one] if r == 0 else [])
        fixed = fixed[:n]
        c = np.sort(np.concatenate([rng.choice(pool, n - len(fixed), replace=False), fixed]).astype(np.int32))
        nf[r] = n
        fcol[r, :n] = c
        fval[r, :n] = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 6, n))
    sval = np.where(rng.random((B, S)) < 0.5, 0, rng.integers(1, 6, (B, S))).astype(np.float32)
    gen = rng.uniform(0.1, 4.9, (B, S)).astype(np.float32)
    zr = ((sval == 0) & (rng.random((B, S)) < 0.5)).astype(np.uint8)
    return dict(fcol=fcol, fval=fval, nf=nf, sval=sval, gen=gen, zr=zr, sel=sel, c_all=c_all if shared else None, c_one=c_one)
