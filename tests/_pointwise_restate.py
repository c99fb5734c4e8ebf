"""NumPy float64 restatement of ONE train step of the two pointwise victims, stage by stage (recad_amd/csrc/ncf.hip: gather, tower
forward, layer dropout, predict + BCE-with-logits, predict backward, predict weight gradient, tower backward, scatter;
recad_amd/csrc/mf.hip: the fused step), the error budget of a correct fp32 implementation of each stage, the seeded cases the host
and the GPU tests share, and a plain fp32 numpy implementation of the step (test_pointwise_ops_host.py shows that it stays inside
every budget and that six wrong implementations do not; test_ncf_kernels_gpu.py / test_mf_kernels_gpu.py hold the kernels to the
budgets).  No GPU, no torch.

Every stage is restated ON THE STAGE'S OWN INPUTS as the implementation under test left them in its workspace (`acts`, `dacts`,
`d0`): a budget is one operation deep, a ReLU gate never has to be guessed (forward: relu is 1-Lipschitz, so a pre-activation within
its budget gives an activation within the same budget on either side of zero; backward: the masks are the workspace's own x > 0),
no element is excluded, and a failure names its stage.

Budgets.  u = 2^-24 is the unit roundoff of fp32.  Nothing below is tuned or measured: every factor counts roundings.
  * gather: a copy, bits.  With dropout fl(v * scale) under the counter mask of tests/_drop_restate.py or +0.0: one fp32 product, bits.
  * a dot product of K terms summed in ANY order (one chain, 8 blocks combined pairwise, K-slices added in order, atomics), each
    product rounded: (K + 8) u sum|a_k b_k| -- K - 1 additions and one product per term, the rest is slack for the bias, a
    second product inside a term (pw * (ug * ig)) and the wave / slice combines.  Tower forward layer l: K = in_l, plus |b|.
  * layer dropout on a stage's output (the workspace only holds the value AFTER it): a kept element is fl(y * scale) with y inside
    its budget B: scale B + 2 u scale |ref| (the product's rounding, and as much again for the cross term); a dropped one is +0.0.
  * predict: the logit is a dot product of PS terms plus pb: ds = (PS + 8) u (sum|pw z| + |pb|).
      sigma = 1 / (1 + expf(-s)): |d sigma / ds| = sigma (1 - sigma), and |d ln sigma' / ds| <= 1 carries it over [s - ds, s + ds]:
      sigma (1 - sigma) e^ds ds; expf is allowed 4 u relative (its effect on sigma is scaled by 1 - sigma <= 1), 1 + e and the
      division one u each: 6 u sigma.  sigma - y is exact for y = 0 and by Sterbenz for sigma >= 1/2, else u |sigma - y|; fl(1 / nb)
      and the product two more: d0 within (sigma (1 - sigma) e^ds ds + 6 u sigma) / nb + 3 u |d0|.
      loss_b = max(s, 0) - s y + log1pf(expf(-|s|)): the first two terms and their difference are exact (y is 0 or 1);
      expf's 4 u passes through log1p as at most 4 u relative (e / (1 + e) <= log1p(e)), log1pf adds its own 4 u, the last
      addition u: 8 u log1p(e^-|s|) + u loss_b; |d loss_b / ds| = |sigma - y| <= |sigma(s) - y| + ds / 4 over the interval.
      The step's loss row is the sum of its RK_LOSS_PARTIALS entries (summed in float64 by the tests): a wave adds
      trips = ceil(nb / (4 grid)) terms, grid = min(256, ceil(nb / 4)), the workgroup three more, fl(1 / nb) and the product two:
      mean_b(per-pair) + (trips + 8) u loss.
    THE 4 u ALLOWANCE FOR expf AND log1pf IS THE ONE FIGURE HERE THAT IS NOT COUNTED: it is taken from the HIP math API's accuracy
    table (1 ulp = 2 u each for expf and log1pf, doubled), not measured.
  * predict backward: dXL[b, k] = xL > 0 ? fl(d0_b pw[off + k]) : +0.0 from the workspace's d0 and xL: one product, bits.
    The GMF table gradients: a row is the sum of n_r atomic terms fl(fl(d0_b pw_k) other_k) in some order; the terms are restated
    in fp32 with their own two roundings, the n_r - 1 additions each round a partial sum of at most A = sum|term|: (n_r + 4) u A.
  * predict weight gradient from the workspace's d0 and z = [ug * ig | xL | 1]: nb products, then the two-stage fixed order
    (rows of a 64-row slab, then the slabs) has nb + slabs additions: (nb + slabs + 8) u sum|d0 z|.
  * tower backward of layer l from the workspace's dY = dacts[l + 1], x = acts[l]: dX = dY W is a dot product of out_l terms,
    (out_l + 8) u sum|dY W|, zero where x <= 0 for l >= 1 (budget 0: exact), with or without K-slices; dW = dY^T x over nb terms:
    (nb + 8) u sum|dY x|; db = column sums over nb terms: (nb + 8) u sum|dY|.  With dropout the mask of layer l once more, as above.
  * scatter from the workspace's dacts[0]: n_r terms without roundings of their own: (n_r + 4) u sum|term|; a row with no
    incidence has budget 0 and must be +0.0, like every tensor a mode does not use.
  * Adam is not restated here: the tests compare bits with the oracle's orc.adam.
  * MF: x = ((<ue, ie> + ub) + ib) + mean: dx_b = (d + 8) u (sum|ue ie| + |ub| + |ib| + |mean|); with dropout x' = fl(x scale) or
    +0.0: scale dx_b + 2 u |x'|.  loss and the coefficient c_b = (sigma - y) / nb * keep as in predict, with one more product for
    keep: 4 u |c_b|, the s-dependent part times scale.  A gradient row is n_r atomic terms fl(c_b other_k), each carrying its
    triplet's coefficient budget and its own rounding: sum_b bc_b |other_k| + (n_r + 4) u sum|term|.  A dropped sample has
    x' = +0.0, loss log 2 and c_b = 0: it contributes exactly zero."""
import math

import numpy as np

from ._drop_restate import _drop_keep, _step_seed

U32 = 2.0 ** -24
LIBM_U = 4                     # relative allowance of the device's expf / log1pf in units of u (module docstring: not measured)
SENTINEL = 7.0
NEUMF, MLP, GMF = 0, 1, 2      # RK_NCF_* (include/recad_hip.h)
MODE_NAMES = {NEUMF: "NeuMF", MLP: "MLP", GMF: "GMF"}
LOSS_PARTIALS = 256            # RK_LOSS_PARTIALS
WGRAD_SLAB = 64                # kWgradSlab (ncf.hip)
INF = float("inf")


# ---------------------------------------------------------------- helpers
def f64(a):
    return np.asarray(a, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over all elements; an element whose budget is zero must be exact, a non-finite one fails"""
    got, ref, bound = np.broadcast_arrays(f64(got), f64(ref), f64(bound))
    err = np.abs(got - ref)
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)) or np.any(err[bound == 0] != 0):
        return INF
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))


def same_bits(got, ref):
    """the `ratio` of a bit-exact stage: 0 or inf"""
    got, ref = np.asarray(got), np.asarray(ref)
    return 0.0 if got.shape == ref.shape and np.array_equal(bits(got), bits(ref)) else INF


def widths(f, L):
    """row width of acts[l] / dacts[l], l = 0 .. L: the input of layer l, and the tower output"""
    return [f << (L - l) for l in range(L)] + [f]


def ps_of(f, mode):
    return 2 * f if mode == NEUMF else f


def tensor_sizes(n_users, n_items, f, L, mode):
    """element counts in the order of rk_ncf_desc.grad[]: ug, ig, um, im, W0.., b0.., pw, pb"""
    E, w = f << (L - 1), widths(f, L)
    return [n_users * f, n_items * f, n_users * E, n_items * E] + [w[l] * (w[l] // 2) for l in range(L)] + [w[l] // 2 for l in range(L)] + [ps_of(f, mode), 1]


def loss_trips(nb):
    return math.ceil(nb / (4 * min(LOSS_PARTIALS, (nb + 3) // 4)))


def score_call(drop_call, chunk):
    return (drop_call << 24) + chunk + (1 << 60)


def drop_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_mask(seed, call, layer, shape, p):
    """keep mask (bool, `shape`) of the Dropout in front of tower layer `layer` in call `call` (ncf.hip drop_spec): element ids in
    row-major order under the seed of step call * 16 + layer (64-bit wrap-around)"""
    step = (call * 16 + layer) & ((1 << 64) - 1)
    return _drop_keep(_step_seed(seed, step), int(np.prod(shape)), 1.0 - float(np.float32(p))).reshape(shape)


def drop32(x, drop, layer):
    """fp32: fl(x * scale) where kept, +0.0 elsewhere; drop = None or (p, seed, call)"""
    x = np.asarray(x, dtype=np.float32)
    if drop is None:
        return x.copy()
    keep = drop_mask(drop[1], drop[2], layer, x.shape, drop[0])
    return np.where(keep, x * drop_scale(drop[0]), np.float32(0.0)).astype(np.float32)


def _drop64(ref, bound, drop, layer):
    if drop is None:
        return ref, bound
    keep, sc = drop_mask(drop[1], drop[2], layer, ref.shape, drop[0]), float(drop_scale(drop[0]))
    ref = np.where(keep, ref * sc, 0.0)
    return ref, np.where(keep, sc * bound + 2 * U32 * np.abs(ref), 0.0)


# ---------------------------------------------------------------- NCF stages
def gather(P, users, items, drop=None):
    """X0[b] = [um[u_b] | im[i_b]] (fp32, bits), under the dropout of layer 0"""
    return drop32(np.concatenate([P["um"][users], P["im"][items]], axis=1), drop, 0)


def tower_forward(x, W, b, drop=None, layer_out=None):
    """relu(x W^T + b) of one layer from ITS input x, under the dropout in front of layer `layer_out` -> (ref, bound)"""
    x, W, b = f64(x), f64(W), f64(b)
    K = W.shape[1]
    ref = np.maximum(x @ W.T + b, 0.0)
    bound = (K + 8) * U32 * (np.abs(x) @ np.abs(W).T + np.abs(b))
    return _drop64(ref, bound, drop, layer_out)


def _predict_z(P, mode, f, users, items, xl):
    gm = f64(P["ug"])[users] * f64(P["ig"])[items]
    return gm if mode == GMF else f64(xl) if mode == MLP else np.concatenate([gm, f64(xl)], axis=1)


def logits(P, mode, f, users, items, xl):
    """-> (s, ds)"""
    t = _predict_z(P, mode, f, users, items, xl) * f64(P["pw"]).reshape(1, -1)
    pb = float(P["pb"].reshape(-1)[0])
    return t.sum(1) + pb, (ps_of(f, mode) + 8) * U32 * (np.abs(t).sum(1) + abs(pb))


def bce(s, ds, y, nb, keep=None, scale=1.0):
    """BCE-with-logits of logits s known to ds -> dict: coef = (sigma - y) / nb (* keep), b_coef, loss (mean), b_loss.
    keep / scale: MF's dropout on the logit (s is the logit AFTER it, ds its budget)"""
    s, ds, y = f64(s), f64(ds), f64(y)
    sig, one_m = np.exp(-np.logaddexp(0.0, -s)), np.exp(-np.logaddexp(0.0, s))
    d = np.where(y > 0, -one_m, sig)
    coef = d / nb
    b_coef = (sig * one_m * np.exp(ds) * ds + (LIBM_U + 2) * U32 * sig) / nb + 3 * U32 * np.abs(coef)
    if keep is not None:
        coef = np.where(keep, coef * scale, 0.0)
        b_coef = np.where(keep, b_coef * scale + U32 * np.abs(coef), 0.0)
    per = np.logaddexp(0.0, s) - s * y
    lp = np.log1p(np.exp(-np.abs(s)))
    b_per = (np.abs(d) + ds / 4) * ds + 2 * LIBM_U * U32 * lp + U32 * per
    loss = float(per.sum() / nb)
    return {"coef": coef, "b_coef": b_coef, "loss": loss, "b_loss": float(b_per.sum() / nb + (loss_trips(nb) + 8) * U32 * loss), "per": per}


def predict_backward(P, mode, f, d0, xl):
    """dXL (fp32, bits) from the workspace's d0 and xL"""
    off = f if mode == NEUMF else 0
    v = np.asarray(d0, dtype=np.float32)[:, None] * np.asarray(P["pw"], dtype=np.float32).reshape(-1)[None, off:off + f]
    return np.where(np.asarray(xl) > 0, v, np.float32(0.0)).astype(np.float32)


def _scatter(rows, terms, n_rows):
    """sum of `terms` (fp32 values, [nb, w]) by row in float64 -> (ref [n_rows, w], bound)"""
    t = f64(terms)
    ref, A, n = np.zeros((n_rows, t.shape[1])), np.zeros((n_rows, t.shape[1])), np.zeros(n_rows)
    np.add.at(ref, rows, t)
    np.add.at(A, rows, np.abs(t))
    np.add.at(n, rows, 1)
    return ref, (n[:, None] + 4) * U32 * A


def gmf_grads(P, f, users, items, d0, n_users, n_items):
    """the GMF tables' gradients from the workspace's d0 -> ((g_ug, bound), (g_ig, bound))"""
    c = np.asarray(d0, dtype=np.float32)[:, None] * np.asarray(P["pw"], dtype=np.float32).reshape(-1)[None, :f]
    return _scatter(users, c * P["ig"][items], n_users), _scatter(items, c * P["ug"][users], n_items)


def predict_wgrad(P, mode, f, users, items, d0, xl, drop_last_slab=False):
    """-> (gpw, bound), (gpb, bound) from the workspace's d0 and xL"""
    d0 = f64(d0)
    nb = len(d0)
    z = np.concatenate([_predict_z(P, mode, f, users, items, xl), np.ones((nb, 1))], axis=1)
    g, mag = d0 @ z, np.abs(d0) @ np.abs(z)
    bound = (nb + math.ceil(nb / WGRAD_SLAB) + 8) * U32 * mag
    return (g[:-1], bound[:-1]), (g[-1:], bound[-1:])


def tower_backward(dy, x, W, l, drop=None):
    """layer l from ITS dY and input x -> dict dX, dW, db: (ref, bound) each"""
    dy, x64, W = f64(dy), f64(x), f64(W)
    nb, out = dy.shape
    dX, bX = dy @ W, (out + 8) * U32 * (np.abs(dy) @ np.abs(W))
    if l >= 1:
        gate = np.asarray(x) > 0
        dX, bX = np.where(gate, dX, 0.0), np.where(gate, bX, 0.0)
    dX, bX = _drop64(dX, bX, drop, l)
    return {"dX": (dX, bX), "dW": (dy.T @ x64, (nb + 8) * U32 * (np.abs(dy).T @ np.abs(x64))),
            "db": (dy.sum(0), (nb + 8) * U32 * np.abs(dy).sum(0))}


def scatter(dx0, users, items, n_users, n_items, E):
    dx0 = np.asarray(dx0)
    return _scatter(users, dx0[:, :E], n_users), _scatter(items, dx0[:, E:], n_items)


# ---------------------------------------------------------------- the workspace of one step, checked stage by stage
def check_ncf_forward(c, ws, drop=None):
    """ws: {"acts": [L + 1 arrays [nb, w_l]], "logits": [nb]} of a scoring chunk over c's pairs -> {stage: ratio}"""
    P, f, L, mode, u, i = c["P"], c["f"], c["L"], c["mode"], c["users"], c["items"]
    r = {}
    if mode != GMF:
        r["gather"] = same_bits(ws["acts"][0], gather(P, u, i, drop))
        for l in range(L):
            ref, bound = tower_forward(ws["acts"][l], P["W"][l], P["b"][l], drop if l + 1 < L else None, l + 1)
            r[f"forward.{l}"] = ratio(ws["acts"][l + 1], ref, bound)
    if "logits" in ws:
        s, ds = logits(P, mode, f, u, i, ws["acts"][L] if mode != GMF else None)
        r["logit"] = ratio(ws["logits"], s, ds)
    return r


def check_ncf_step(c, ws, drop=None, nb_div=None):
    """ws: {"acts", "dacts": [L + 1 arrays [nb, w_l]], "d0": [nb], "grad": [T arrays in tensor order], "loss": the step's loss row
    summed in float64} as one apply_update = 0 step over c's pairs left them -> {stage: worst err / bound}"""
    P, f, L, mode, u, i, y = c["P"], c["f"], c["L"], c["mode"], c["users"], c["items"], c["labels"]
    nb, nu, ni, E = len(u), c["n_users"], c["n_items"], f << (L - 1)
    g = [np.asarray(a) for a in ws["grad"]]
    r = check_ncf_forward(c, {"acts": ws["acts"]}, drop)
    xl = ws["acts"][L] if mode != GMF else None
    s, ds = logits(P, mode, f, u, i, xl)
    pr = bce(s, ds, y, nb if nb_div is None else nb_div)
    r["predict.d0"] = ratio(ws["d0"], pr["coef"], pr["b_coef"])
    r["predict.loss"] = abs(float(ws["loss"]) - pr["loss"]) / pr["b_loss"] if np.isfinite(ws["loss"]) else INF
    zero = lambda a: 0.0 if not np.any(bits(a)) else INF
    if mode != MLP:
        (rug, bug), (rig, big) = gmf_grads(P, f, u, i, ws["d0"], nu, ni)
        r["predict.g_ug"], r["predict.g_ig"] = ratio(g[0].reshape(nu, f), rug, bug), ratio(g[1].reshape(ni, f), rig, big)
        untouched = lambda a, rows: a.reshape(-1, f)[np.setdiff1d(np.arange(a.size // f), rows)]
        r["predict.gmf_untouched"] = max(zero(untouched(g[0], u)), zero(untouched(g[1], i)))
    else:
        r["unused.gmf"] = max(zero(g[0]), zero(g[1]))
    (rpw, bpw), (rpb, bpb) = predict_wgrad(P, mode, f, u, i, ws["d0"], xl)
    r["wgrad.pw"], r["wgrad.pb"] = ratio(g[4 + 2 * L].reshape(-1), rpw, bpw), ratio(g[5 + 2 * L].reshape(-1), rpb, bpb)
    if mode == GMF:
        r["unused.tower"] = max(zero(a) for a in g[2:4 + 2 * L])
        return r
    r["predict.dxl"] = same_bits(ws["dacts"][L], predict_backward(P, mode, f, ws["d0"], xl))
    for l in range(L - 1, -1, -1):
        t = tower_backward(ws["dacts"][l + 1], ws["acts"][l], P["W"][l], l, drop)
        r[f"backward.{l}.dX"] = ratio(ws["dacts"][l], *t["dX"])
        r[f"backward.{l}.dW"] = ratio(g[4 + l].reshape(t["dW"][0].shape), *t["dW"])
        r[f"backward.{l}.db"] = ratio(g[4 + L + l].reshape(-1), *t["db"])
    (rum, bum), (rim, bim) = scatter(ws["dacts"][0], u, i, nu, ni, E)
    r["scatter.um"], r["scatter.im"] = ratio(g[2].reshape(nu, E), rum, bum), ratio(g[3].reshape(ni, E), rim, bim)
    um_free, im_free = np.setdiff1d(np.arange(nu), u), np.setdiff1d(np.arange(ni), i)
    r["scatter.untouched"] = max(zero(g[2].reshape(nu, E)[um_free]), zero(g[3].reshape(ni, E)[im_free]))
    return r


# ---------------------------------------------------------------- the whole step in float64 (for autograd) and in plain fp32
def ncf_step64(c, masks=None, p=0.0):
    """one step chained in float64 (each stage fed with the previous stage's float64 output) -> (loss, [T gradients]); masks: one
    keep mask [nb, w_l] per layer, applied with 1 / (1 - p)"""
    P, f, L, mode, u, i, y = c["P"], c["f"], c["L"], c["mode"], c["users"], c["items"], c["labels"]
    nb, nu, ni, E = len(u), c["n_users"], c["n_items"], f << (L - 1)
    sc = 1.0 / (1.0 - p)
    drop = (lambda a, l: a) if masks is None else (lambda a, l: a * masks[l] * sc)
    acts = [drop(np.concatenate([f64(P["um"])[u], f64(P["im"])[i]], axis=1), 0)]
    for l in range(L):
        a = np.maximum(acts[l] @ f64(P["W"][l]).T + f64(P["b"][l]), 0.0)
        acts.append(drop(a, l + 1) if l + 1 < L else a)
    xl = acts[L] if mode != GMF else None
    s, _ = logits(P, mode, f, u, i, xl)
    pr = bce(s, 0 * s, y, nb)
    d0, pw = pr["coef"], f64(P["pw"]).reshape(-1)
    z = _predict_z(P, mode, f, u, i, xl)
    grads = [np.zeros(n) for n in tensor_sizes(nu, ni, f, L, mode)]
    if mode != MLP:
        gu, gi = np.zeros((nu, f)), np.zeros((ni, f))
        np.add.at(gu, u, d0[:, None] * pw[:f] * f64(P["ig"])[i])
        np.add.at(gi, i, d0[:, None] * pw[:f] * f64(P["ug"])[u])
        grads[0], grads[1] = gu.reshape(-1), gi.reshape(-1)
    grads[4 + 2 * L], grads[5 + 2 * L] = d0 @ z, np.array([d0.sum()])
    if mode != GMF:
        off = f if mode == NEUMF else 0
        dy = np.where(acts[L] > 0, d0[:, None] * pw[off:off + f], 0.0)
        for l in range(L - 1, -1, -1):
            grads[4 + l], grads[4 + L + l] = (dy.T @ acts[l]).reshape(-1), dy.sum(0)
            dx = dy @ f64(P["W"][l])
            if l >= 1:                  # relu' of the layer below: its output is > 0 wherever the (kept) activation is
                dx = np.where(acts[l] > 0, dx, 0.0)
            dy = drop(dx, l)
        gum, gim = np.zeros((nu, E)), np.zeros((ni, E))
        np.add.at(gum, u, dy[:, :E])
        np.add.at(gim, i, dy[:, E:])
        grads[2], grads[3] = gum.reshape(-1), gim.reshape(-1)
    return pr["loss"], grads


def _mm32(a, b, reverse):
    """a [m, k] . b [n, k]^T with fp32 accumulation; reverse: the k axis summed from the other end"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a[:, ::-1] @ b[:, ::-1].T if reverse else a @ b.T).astype(np.float32)


def _add_at32(n_rows, rows, terms, reverse, skip=None):
    out = np.zeros((n_rows, terms.shape[1]), dtype=np.float32)
    order = np.arange(len(rows))[::-1] if reverse else np.arange(len(rows))
    if skip is not None:
        order = order[order != skip]
    np.add.at(out, rows[order], terms[order].astype(np.float32))
    return out


def _loss32(per, inv, reverse):
    """the loss row as the kernels lay it out: wave w of 4 * grid adds the pairs w, w + 4 grid, .. in fp32, a workgroup its four waves,
    times fl(1 / nb); the partials are summed in float64 as the tests sum a device loss row"""
    nb = len(per)
    waves = 4 * min(LOSS_PARTIALS, (nb + 3) // 4)
    sums = np.zeros(waves, dtype=np.float32)
    for t in (range(loss_trips(nb) - 1, -1, -1) if reverse else range(loss_trips(nb))):
        part = per[t * waves:(t + 1) * waves]
        sums[:len(part)] = sums[:len(part)] + part
    r = sums.reshape(-1, 4)
    return float((((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) * inv).astype(np.float64).sum())


def ncf_step32(c, drop=None, reverse=False, mutate=None, nb_div=None):
    """one step in plain fp32 numpy, the sums of every stage in index order or (reverse) from the other end -> the workspace dict
    check_ncf_step takes.  mutate: one of the wrong implementations of test_pointwise_ops_host.py"""
    P, f, L, mode, u, i, y = c["P"], c["f"], c["L"], c["mode"], c["users"], c["items"], c["labels"]
    nb, nu, ni, E, w = len(u), c["n_users"], c["n_items"], f << (L - 1), widths(f, L)
    one = np.float32(1.0)
    PS = ps_of(f, mode)
    pw, pb = np.asarray(P["pw"], dtype=np.float32).reshape(-1), np.float32(P["pb"].reshape(-1)[0])
    if mutate == "pw_halves" and mode == NEUMF:
        pw = np.concatenate([pw[f:], pw[:f]])
    acts, pre, dacts = [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
    grad = [np.zeros(n, dtype=np.float32) for n in tensor_sizes(nu, ni, f, L, mode)]
    if mode != GMF:
        x0 = np.concatenate([P["um"][u], P["im"][i]], axis=1)
        acts[0] = drop32(x0, drop, 1 if mutate == "seed_layer" else 0)
        for l in range(L):
            pre[l + 1] = np.maximum(_mm32(acts[l], P["W"][l], reverse) + P["b"][l], np.float32(0.0)).astype(np.float32)
            acts[l + 1] = drop32(pre[l + 1], drop, l + 1) if l + 1 < L else pre[l + 1]
    gm = (P["ug"][u] * P["ig"][i]).astype(np.float32)
    z = gm if mode == GMF else acts[L] if mode == MLP else np.concatenate([gm, acts[L]], axis=1)
    s = (_mm32(z, pw[None, :], reverse)[:, 0] + pb).astype(np.float32)
    yf = y.astype(np.float32)
    inv = one / np.float32(nb if nb_div is None else nb_div)
    with np.errstate(over="ignore"):
        per = (np.maximum(s, 0) - s * yf + np.log1p(np.exp(-np.abs(s)))).astype(np.float32)
        d0 = ((one / (one + np.exp(-s)) - yf) * inv).astype(np.float32)
    loss = _loss32(per, inv, reverse)
    if mode != MLP:
        cf = d0[:, None] * pw[None, :f]
        grad[0] = _add_at32(nu, u, cf * P["ig"][i], reverse).reshape(-1)
        grad[1] = _add_at32(ni, i, cf * P["ug"][u], reverse).reshape(-1)
    z1 = np.concatenate([z, np.ones((nb, 1), dtype=np.float32)], axis=1)
    n_slabs = math.ceil(nb / WGRAD_SLAB)
    slabs = [(_mm32(z1[q * WGRAD_SLAB:(q + 1) * WGRAD_SLAB].T, d0[None, q * WGRAD_SLAB:(q + 1) * WGRAD_SLAB], reverse)[:, 0]) for q in range(n_slabs)]
    if mutate == "last_slab":
        slabs = slabs[:-1]
    gp = np.zeros(PS + 1, dtype=np.float32)
    for part in (slabs[::-1] if reverse else slabs):
        gp = (gp + part).astype(np.float32)
    grad[4 + 2 * L], grad[5 + 2 * L] = gp[:PS].copy(), gp[PS:].copy()
    if mode != GMF:
        off = f if mode == NEUMF else 0
        dacts[L] = np.where(acts[L] > 0, d0[:, None] * pw[None, off:off + f], np.float32(0.0)).astype(np.float32)
        for l in range(L - 1, -1, -1):
            dy = dacts[l + 1]
            grad[4 + l] = _mm32(dy.T, acts[l].T, reverse).reshape(-1)
            col = np.zeros(dy.shape[1], dtype=np.float32)
            for row in (dy[::-1] if reverse else dy):
                col = (col + row).astype(np.float32)
            grad[4 + L + l] = col
            dx = _mm32(dy, P["W"][l].T, reverse)
            if mutate == "pre_dropout_mask" and drop is not None and l >= 1:
                # the gate from the activation BEFORE its dropout, the zeroing of the dropped entries left to that gate
                dx = (np.where(pre[l] > 0, dx, np.float32(0.0)) * drop_scale(drop[0])).astype(np.float32)
            else:
                if l >= 1:
                    dx = np.where(acts[l] > 0, dx, np.float32(0.0)).astype(np.float32)
                dx = drop32(dx, drop, l)
            dacts[l] = dx
        skip = nb // 2 if mutate == "scatter_pair" else None
        grad[2] = _add_at32(nu, u, dacts[0][:, :E], reverse, skip).reshape(-1)
        grad[3] = _add_at32(ni, i, dacts[0][:, E:], reverse).reshape(-1)
    return {"acts": acts, "dacts": dacts, "d0": d0, "grad": grad, "loss": loss, "logits": s}


# ---------------------------------------------------------------- MF
def mf_step(c, drop=None, nb_div=None):
    """mf_step_kernel in float64 -> {"loss", "b_loss", "grad": [(ref, bound)] * 4 for ue, ie, ub, ib, "keep"}; drop = (p, seed, step)"""
    ue, ie, ub, ib, u, i, y = c["ue"], c["ie"], c["ub"], c["ib"], c["users"], c["items"], c["labels"]
    nb, d, nu, ni = len(u), c["dim"], c["n_users"], c["n_items"]
    t = f64(ue)[u] * f64(ie)[i]
    bu, bi, mean = f64(ub)[u], f64(ib)[i], float(np.float32(c["mean"]))
    x = t.sum(1) + bu + bi + mean
    dx = (d + 8) * U32 * (np.abs(t).sum(1) + np.abs(bu) + np.abs(bi) + abs(mean))
    keep, sc = None, 1.0
    if drop is not None:
        keep, sc = _drop_keep(_step_seed(drop[1], drop[2]), nb, 1.0 - float(np.float32(drop[0]))), float(drop_scale(drop[0]))
        x = np.where(keep, x * sc, 0.0)
        dx = np.where(keep, sc * dx + 2 * U32 * np.abs(x), 0.0)
    pr = bce(x, dx, y, nb if nb_div is None else nb_div, keep, sc)
    cf, bc = pr["coef"], pr["b_coef"]
    out = []
    for rows, other, n_rows in ((u, ie[i], nu), (i, ue[u], ni), (u, np.ones((nb, 1), np.float32), nu), (i, np.ones((nb, 1), np.float32), ni)):
        terms = cf[:, None] * f64(other)
        ref, b_sum = _scatter(rows, terms, n_rows)
        W = np.zeros_like(ref)
        np.add.at(W, rows, bc[:, None] * np.abs(f64(other)) + U32 * np.abs(terms))
        out.append((ref, W + b_sum))
    return {"loss": pr["loss"], "b_loss": pr["b_loss"], "grad": out, "keep": keep, "x": x}


def check_mf_step(c, grads, loss, drop=None, nb_div=None):
    """grads: the flat [U d | I d | U | I] buffer after one apply_update = 0 step, loss: its loss row summed in float64"""
    ref = mf_step(c, drop, nb_div)
    d, nu, ni = c["dim"], c["n_users"], c["n_items"]
    g = np.asarray(grads)
    parts = (g[:nu * d].reshape(nu, d), g[nu * d:(nu + ni) * d].reshape(ni, d), g[(nu + ni) * d:(nu + ni) * d + nu].reshape(nu, 1),
             g[(nu + ni) * d + nu:].reshape(ni, 1))
    r = {"mf.loss": abs(float(loss) - ref["loss"]) / ref["b_loss"] if np.isfinite(loss) else INF}
    for name, got, (want, bound), rows in zip(("ue", "ie", "ub", "ib"), parts, ref["grad"], (c["users"], c["items"]) * 2):
        r[f"mf.g_{name}"] = ratio(got, want, bound)
        live = rows if ref["keep"] is None else rows[ref["keep"]]
        free = np.setdiff1d(np.arange(len(got)), live)
        r[f"mf.g_{name}.untouched"] = 0.0 if not np.any(bits(got[free])) else INF
    return r


def mf_step32(c, drop=None, reverse=False, mutate=None, nb_div=None):
    """the MF step in plain fp32 numpy -> (flat gradient buffer, loss)"""
    ue, ie, ub, ib, u, i, y = c["ue"], c["ie"], c["ub"], c["ib"], c["users"], c["items"], c["labels"]
    nb, nu, ni, one = len(u), c["n_users"], c["n_items"], np.float32(1.0)
    pu, pi = ue[u], ie[i]
    prod = (pu * pi).astype(np.float32)
    s = (prod[:, ::-1] if reverse else prod).astype(np.float32) @ np.ones(prod.shape[1], dtype=np.float32)
    x = (((s + ub[u]) + ib[i]) + np.float32(c["mean"])).astype(np.float32)
    keep = np.ones(nb, dtype=np.float32)
    if drop is not None:
        keep = np.where(_drop_keep(_step_seed(drop[1], drop[2]), nb, 1.0 - float(np.float32(drop[0]))), drop_scale(drop[0]), np.float32(0.0)).astype(np.float32)
        x = (x * keep).astype(np.float32)
    yf, inv = y.astype(np.float32), one / np.float32(nb if nb_div is None else nb_div)
    with np.errstate(over="ignore"):
        per = (np.maximum(x, 0) - x * yf + np.log1p(np.exp(-np.abs(x)))).astype(np.float32)
        dx = ((one / (one + np.exp(-x)) - yf) * inv * keep).astype(np.float32)
    loss = _loss32(per, inv, reverse)
    skip = nb // 2 if mutate == "scatter_pair" else None
    g = [_add_at32(nu, u, dx[:, None] * pi, reverse, skip), _add_at32(ni, i, dx[:, None] * pu, reverse),
         _add_at32(nu, u, dx[:, None], reverse), _add_at32(ni, i, dx[:, None], reverse)]
    return np.concatenate([a.reshape(-1) for a in g]), loss


# ---------------------------------------------------------------- seeded cases
HUB_USER, HUB_ITEM, BIG = 150, 90, 40.0


def batch(nb, n_users, n_items, rng, hubs=True):
    """users / items / labels of nb pairs: all distinct, or (hubs, nb >= 5) pairs 0 and 1 on rows of their own (the +-40 logits), one
    user in min(150, nb - 2) pairs from pair 2 on and one item in the last min(90, nb - 2) pairs, everything else distinct"""
    assert n_users >= nb and n_items >= nb
    u, i = rng.permutation(n_users)[:nb].astype(np.int64), rng.permutation(n_items)[:nb].astype(np.int64)
    y = rng.integers(0, 2, size=nb).astype(np.int64)
    if hubs and nb >= 5:
        u[2:2 + min(HUB_USER, nb - 2)] = u[2]
        i[nb - min(HUB_ITEM, nb - 2):] = i[nb - 1]
        y[:2] = 0
    return u, i, y


def _pair_logit(P, f, L, mode, rows):
    """float64 logit of one pair from its four (fp32) table rows, no dropout"""
    ug, ig, um, im = (f64(r) for r in rows)
    x = np.concatenate([um, im])
    for l in range(L):
        x = np.maximum(f64(P["W"][l]) @ x + f64(P["b"][l]), 0.0)
    z = ug * ig if mode == GMF else x if mode == MLP else np.concatenate([ug * ig, x])
    return float(f64(P["pw"]).reshape(-1) @ z + float(P["pb"].reshape(-1)[0]))


def _aim_pair(P, f, L, mode, u, i, target, rng):
    """scale the four table rows of pair (u, i) by one factor c so that its logit is within 0.5 of target: the logit is continuous
    in c, so bisect between a factor short of the target and one past it; rows whose logit cannot take the target's sign are redrawn"""
    E = f << (L - 1)
    for _ in range(400):
        base = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (f, f, E, E)]
        g = lambda c: _pair_logit(P, f, L, mode, [(np.float32(c) * r).astype(np.float32) for r in base])
        past = lambda c: (g(c) - target) * np.sign(target) > 0
        lo, hi = 0.0, 1.0
        while not past(hi) and hi < 4096:
            lo, hi = hi, 2 * hi
        if not past(hi):
            continue
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if past(mid) else (mid, hi)
            if abs(g(hi) - target) < 0.5:
                break
        if abs(g(hi) - target) < 0.5:
            for name, r in zip(("ug", "ig", "um", "im"), base):
                P[name][u if name[0] == "u" else i] = (np.float32(hi) * r).astype(np.float32)
            return
    raise AssertionError("no +-40 pair found")


def ncf_case(f, L, mode, nb, seed, n_users=None, n_items=None, hubs=True):
    """parameters (embeddings 0.3 N(0, 1), Xavier-uniform tower weights, biases uniform in +-0.05, the predict layer Xavier-uniform
    with both signs in each half) and one batch (batch()); with hubs and nb >= 5, pairs 0 / 1 have logits +40 / -40"""
    rng = np.random.default_rng(seed)
    nu, ni = n_users or nb + 8, n_items or nb + 6
    E, w, PS = f << (L - 1), widths(f, L), ps_of(f, mode)
    n = lambda *s: (0.3 * rng.standard_normal(s)).astype(np.float32)
    xav = lambda o, k: rng.uniform(-1, 1, size=(o, k)).astype(np.float32) * np.float32(math.sqrt(6.0 / (o + k)))
    P = {"ug": n(nu, f), "ig": n(ni, f), "um": n(nu, E), "im": n(ni, E), "W": [xav(w[l] // 2, w[l]) for l in range(L)],
         "b": [rng.uniform(-0.05, 0.05, size=w[l] // 2).astype(np.float32) for l in range(L)], "pw": xav(1, PS).reshape(-1),
         "pb": rng.uniform(-0.05, 0.05, size=1).astype(np.float32)}
    for h in range(PS // f):                      # both signs in each half: both targets are reachable through the ReLU outputs
        P["pw"][h * f], P["pw"][h * f + 1] = abs(P["pw"][h * f]), -abs(P["pw"][h * f + 1])
    u, i, y = batch(nb, nu, ni, rng, hubs)
    c = {"f": f, "L": L, "mode": mode, "nb": nb, "n_users": nu, "n_items": ni, "P": P, "users": u, "items": i, "labels": y, "big": hubs and nb >= 5}
    if c["big"]:
        _aim_pair(P, f, L, mode, u[0], i[0], BIG, rng)
        _aim_pair(P, f, L, mode, u[1], i[1], -BIG, rng)
    return c


def ncf_tensors(c):
    """the parameters in the order of rk_ncf_desc.grad[]"""
    P = c["P"]
    return [P["ug"], P["ig"], P["um"], P["im"]] + list(P["W"]) + list(P["b"]) + [P["pw"], P["pb"]]


def sub_case(c, lo, hi):
    """the same model over pairs lo .. hi - 1"""
    s = dict(c)
    s.update(users=c["users"][lo:hi], items=c["items"][lo:hi], labels=c["labels"][lo:hi], nb=hi - lo)
    return s


def mf_case(dim, nb, seed, n_users=None, n_items=None, hubs=True, mean=0.37):
    rng = np.random.default_rng(seed)
    nu, ni = n_users or nb + 8, n_items or nb + 6
    n = lambda *s: (0.3 * rng.standard_normal(s)).astype(np.float32)
    c = {"dim": dim, "nb": nb, "n_users": nu, "n_items": ni, "ue": n(nu, dim), "ie": n(ni, dim), "ub": n(nu), "ib": n(ni), "mean": mean}
    c["users"], c["items"], c["labels"] = batch(nb, nu, ni, rng, hubs)
    c["big"] = hubs and nb >= 5
    if c["big"]:
        for b, target in ((0, BIG), (1, -BIG)):
            u, i = c["users"][b], c["items"][b]
            row = f64(c["ue"][u])
            rest = float(c["ub"][u]) + float(c["ib"][i]) + float(np.float32(mean))
            c["ie"][i] = ((target - rest) / (row * row).sum() * row).astype(np.float32)
    return c


# the case table of tests/test_ncf_kernels_gpu.py: name -> (factor, L, mode, nb, dropout)
NCF_CASES = {f"A{nb}": (4, 1, NEUMF, nb, 0.0) for nb in (1, 3, 4, 5, 64, 65)}
NCF_CASES.update({"B": (4, 8, MLP, 70, 0.0), "C": (64, 3, NEUMF, 200, 0.0), "Cdrop": (64, 3, NEUMF, 200, 0.3),
                  "Dgmf": (32, 2, GMF, 1100, 0.0), "Dmlp": (32, 2, MLP, 1100, 0.0), "E": (64, 1, MLP, 65, 0.0)})
DROP_SEED = 0x5EED1234ABCD
MF_DIMS, MF_NB, MF_DROPS = (1, 63, 64, 65, 130), (1, 5, 1025, 1100), (0.0, 0.25)
_memo = {}


def named_case(name):
    """the shared, never modified case of a row of the table"""
    if name not in _memo:
        f, L, mode, nb, p = NCF_CASES[name]
        _memo[name] = ncf_case(f, L, mode, nb, seed=1000 * f + 10 * L + mode + nb)
    return _memo[name]


def named_mf_case(dim, nb):
    if ("mf", dim, nb) not in _memo:
        _memo["mf", dim, nb] = mf_case(dim, nb, seed=77 * dim + nb)
    return _memo["mf", dim, nb]
