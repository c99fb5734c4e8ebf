"""NumPy float64 restatement of the AushPlus kernels (recad_amd/csrc/aushplus.hip: rk_ap_g_forward, rk_ap_g_backward,
rk_ap_d_step) STAGE BY STAGE, the error budget of a correct fp32 implementation of each stage, the one seeded case the host and
the GPU tests share, and a plain fp32 numpy implementation of every stage with ten switchable mistakes
(test_aushplus_stages_host.py shows that the fp32 implementation stays inside every budget in both summation orders and that
each mistake does not; test_aushplus_kernels_gpu.py holds the kernels to the budgets).  No GPU.  tests/_aushplus_restate.py
stays the autograd form of the same model; the host test shows that the stages chained in float64 equal it.

Every stage is restated ON THE STAGE'S OWN INPUTS as the implementation under test left them in the caller's buffers (norm, h1,
a, zbar, bbar, dpre; D's work arrays): a budget is one operation deep, a relu gate or a Heaviside never has to be guessed (the
gates are the buffers' own h > 0, the Heavisides the signs of a - b_k with the fp32 boundaries, and the sign of a correctly
rounded fp32 difference is the sign of the exact one), no element is excluded, and a failure names its stage.  A stage function
returns (reference, bound) per element; a bound of 0 demands the value exactly.

Budgets.  u = 2^-24 is the unit roundoff of fp32.  Nothing below is tuned or measured: every factor counts roundings, to first
order in u, and the integer slack written next to each count pays for the second order.  The build passes no fast-math flag, so
sqrtf and / are correctly rounded: one u each.
THE ALLOWANCE OF 4 u FOR tanhf, expf AND logf (T BELOW) IS THE ONE FIGURE HERE THAT IS NOT COUNTED: like expf and log1pf in
tests/_pointwise_restate.py it is taken from the HIP math API's accuracy table (1 ulp = 2 u for each, doubled), not measured.
  * a dot product of K terms summed in ANY order, each product rounded (or fused, which only removes a rounding): a term passes
    its own product and at most K - 1 additions, so K u sum|terms|; written (K + c) u sum|terms| with c = 2 for one chain and
    c = 8 where lanes are combined by wave_sum (six more additions on a path, the bias, the in-lane pair).
  G forward
  * norm = max(sqrtf(s2), 1e-12f), s2 the K-term sum of x^2: K u relative on s2 (all terms >= 0), halved by the square root, one
    u for sqrtf: (K / 2 + 2) u norm.  An empty (or all-zero) row gives the float 1e-12f exactly.
  * h1 = relu(acc / norm + b1) from the device's norm: acc is a K-term dot product, the division and the addition one u each:
    (K + 4) u (sum|x w| / norm + |b1|); relu is 1-Lipschitz.  A padding lane (w = b = 0) has budget 0.
  * a = fl(fl(tanhf(z)) 2.5f) + 2.5f, z = W2_j . h1 + b2_j over the 128 lanes from the device's h1: dz = (128 + 8) u
    (sum|w h| + |b2|); carried through 2.5 tanh with the largest slope on [z - dz, z + dz], 2.5 sech^2(max(|z| - dz, 0)) dz;
    tanhf's T u |tanh z| times 2.5, the product's u 2.5 |tanh z| and one more for the second order, the addition's u |a|:
    2.5 sech^2(..) dz + (T + 2) u 2.5 |tanh z| + u |a|.
  * cls, value from the device's a: the boundaries restated in fp32 with every operation rounded on its own (b0 = min_boundary,
    cur = fl(max(len, 0) + 1e-4f), b_k = fl(b_{k-1} + cur)), d_k = fl(a - b_k), the four strict comparisons: bits, no margin.
  G backward, per row, from the device's a, x, dvalue / scale and the fp32 boundaries
  * gc_c: mode 0 fl((c + 1) dv), dv = dvalue [x > 0]: u |gc|.  mode 1, the five 0/1 products as logits: se = sum_c expf(dist_c)
    (T + 4) u relative (five expf, four additions); lse = logf(se): dlse = (T + 4) u + T u |lse|; p_c = expf(dist_c - lse):
    the argument carries dlse and its own u |dist_c - lse|, expf T u: dp = p (dlse + u |arg| + T u); gc = fl(fl(p - [c = y])
    scale): scale dp + 2 u |gc|; eloss = fl(fl(lse - dist_y) scale): scale dlse + 2 u |eloss|.  Entries with x <= 0 (or a
    rating outside 1..5) give gc = 0 and eloss = 0 exactly.
  * sech2_k = 1 - th^2, th = tanhf(fl(a - b_k)): dth = T u |th| + u |d| sech^2(d); ds = 2 |th| dth + u th^2 + u sech2.
  * dd_k = sum over the at most five classes whose other three factors hold of s_ck gc_c sech2_k (the Heaviside products are 0/1:
    exact): sum_c (dgc_c sech2 + |gc_c| ds) + (5 + 1) u sum|terms|; bbar_k = -dd_k exactly.
  * abar = sum_k dd_k: sum_k ddd_k + 4 u sum|dd|.  h2 = fl(fl(a - 2.5f) / 2.5f): 2 u |h2|; q = 1 - h2^2: 5 u h2^2 + u |q|
    (2 |h2| 2 u |h2|, the square, the difference); zbar = fl(fl(abar 2.5f) q): 2.5 (dabar |q| + |abar| dq) + 3 u |zbar|.
  * dpre = [h1 > 0] sum_k zbar_k w2[col_k] from the device's zbar and h1, one chain: (K + 2) u sum|terms|; +0.0 where h1 <= 0.
  G backward, per item through the transposed list (n_j entries), from the device's zbar, bbar, dpre, h1, norm
  * w2-bar = sum zbar h1: (n_j + 2) u sum|terms|; w1t-bar = sum fl(x / norm) dpre, one more rounding per term: (n_j + 3) u
    sum|terms|.  The compiler may contract these multiply-adds, hence a budget.
  * ADDITIONS IN A WRITTEN ORDER, walked in fp32 and compared bit for bit: b2-bar = the chain of zbar in list order; min_boundary-
    bar = the chain of ((bbar0 + bbar1) + bbar2) + bbar3; interval_lengths-bar_m = the chain of the tail sums of bbar from m + 1
    on, +0.0 where len <= 0; b1-bar = colsum_kernel: the chain of dpre over the rows in row order; loss[0] = sum_kernel: 256
    partials (thread t chains in[t], in[t + 256], ...), then the halving tree red[t] += red[t + o], o = 128 ... 1.
  D, from the device's work arrays
  * h1 = relu(sum val w1t + b1), one chain: (K + 2) u (sum|v w| + |b1|).  h2 = relu(W2 h1 + b2), 512 terms over the lanes of a
    wave: (512 + 8) u (sum|W h| + |b2|).  logit s from the device's h2: ds = (128 + 8) u (sum|w3 h2| + |b3|); p = 1 / (1 +
    expf(-s)): sigma (1 - sigma) e^ds ds + (T + 2) u sigma (expf, the addition, the division) + 2^-126: below the smallest
    normal number expf's overflow makes p exactly 0.
  * rowloss from the device's p: l = -(y max(logf(p), -100) + (1 - y) max(logf(fl(1 - p)), -100)), y in {0, 1} so products and
    sum are exact: y = 1: T u |log p|; y = 0: u (the rounding of 1 - p, through log) + T u |log(1 - p)|; the clamp is
    1-Lipschitz; rowloss = fl(l fl(1 / n_side)): dl / n_side + 2 u |rowloss|.
  * dlogit = fl(fl(fl(fl(p - y) / max(fl(fl(1 - p) p), 1e-12f)) fl(p fl(1 - p))) fl(1 / n_side)): nine roundings, (9 + 1) u
    |dlogit|; exactly 0 when p is 0 or 1.
  * dz2 = [h2 > 0] fl(dlogit w3) from the device's dlogit and h2: one product, bits, +0.0 under the gate.  dz1 = [h1 > 0] sum_u
    dz2_u W2[u], one chain of 128: (128 + 2) u sum|terms|, +0.0 under the gate.  dinB = w1t[col] . dz1 over the lanes of a
    wave: (512 + 8) u sum|terms|.
  * W2-bar, w3-bar over the n rows: (n + 2) u sum|terms|; w1t-bar of item j over its n_j entries: (n_j + 2) u sum|terms|;
    b2-bar, b1-bar, b3-bar are chains of additions in row order and loss[0] is sum_kernel over rowloss: bits."""
import numpy as np

U = 2.0 ** -24
T = 4                          # allowance of the device's tanhf / expf / logf in units of u (module docstring: not measured)
TINY = 2.0 ** -126
SENTINEL = 7.0
SENT_BITS = np.float32(SENTINEL).view(np.uint32)
HG, HGR, HD1, HD2 = 128, 125, 512, 128
INF = float("inf")
F32 = np.float32
EPS12 = float(F32(1e-12))
EPS4 = F32(1e-4)
SGN = np.where(np.arange(4)[None, :] < np.arange(5)[:, None], 1.0, -1.0)        # s_ck, [5, 4]

MUTANTS = ("dinb_first8", "rowback_first128", "value_nomask", "dvalue_nomask", "no_eps", "ge", "bce_weight", "ilen_nogate",
           "entry0_ignored", "norm_unclamped")


# ---------------------------------------------------------------- helpers
def f64(a):
    return np.asarray(a, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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
    return 0.0 if got.shape == ref.shape and got.dtype.itemsize == 4 == ref.dtype.itemsize and np.array_equal(bits(got), bits(ref)) else INF


def plus_zero(got, mask):
    """0 when every element of got under mask is +0.0 in bits, else inf"""
    return 0.0 if not np.any(bits(np.asarray(got, dtype=F32))[np.broadcast_to(mask, np.shape(got))]) else INF


def all_sentinel(a):
    return bool(np.all(bits(a) == SENT_BITS))


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _seg(n, rows, t):
    out = np.zeros((n,) + t.shape[1:])
    np.add.at(out, rows, t)
    return out


def _r32(a):
    return np.asarray(a, dtype=np.float64).astype(F32)


def _dot(terms, reverse=False):
    """sum over the LAST axis in one fp32 chain from +0, front to back or back to front"""
    terms = np.asarray(terms, dtype=F32)
    terms = np.concatenate([np.zeros(terms.shape[:-1] + (1,), dtype=F32), terms[..., ::-1] if reverse else terms], axis=-1)
    return np.cumsum(terms, axis=-1, dtype=F32)[..., -1]


# ---------------------------------------------------------------- additions in a written order (dtype float32: the kernels' bits)
def colsum(mat, dtype=F32):
    """colsum_kernel: out[t] = the chain over the rows, in row order, from +0"""
    mat = np.asarray(mat, dtype=dtype)
    return np.cumsum(np.concatenate([np.zeros((1,) + mat.shape[1:], dtype), mat]), axis=0, dtype=dtype)[-1]


def sum_kernel(v, dtype=F32):
    """sum_kernel: thread t chains v[t], v[t + 256], ... from +0; then red[t] += red[t + o] for o = 128, 64 ... 1"""
    v = np.asarray(v, dtype=dtype).reshape(-1)
    red = colsum(np.concatenate([v, np.zeros(-len(v) % 256, dtype)]).reshape(-1, 256), dtype).copy()
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0]


def side_sums(I, tptr, tent, zbar, bbar, ilen, dtype=F32, gate=True):
    """b2-bar [I], min_boundary-bar [I], interval_lengths-bar [I, 3]: the chains of g_item_backward_kernel's threads 0 .. 4"""
    zbar, bbar = np.asarray(zbar, dtype=dtype), np.asarray(bbar, dtype=dtype).reshape(-1, 4)
    gb2, gminb, gilen = np.zeros(I, dtype), np.zeros(I, dtype), np.zeros((I, 3), dtype)
    for j in range(I):
        s = [dtype(0)] * 5
        for q in range(tptr[j], tptr[j + 1]):
            k = tent[q]
            b = bbar[k]
            s[0] = s[0] + zbar[k]
            s[1] = s[1] + (((b[0] + b[1]) + b[2]) + b[3])
            s[2] = s[2] + ((b[1] + b[2]) + b[3])
            s[3] = s[3] + (b[2] + b[3])
            s[4] = s[4] + b[3]
        gb2[j], gminb[j] = s[0], s[1]
        for m in range(3):
            gilen[j, m] = s[2 + m] if (ilen[j, m] > 0 or not gate) else dtype(0)
    return gb2, gminb, gilen


# ---------------------------------------------------------------- boundaries and classes
def boundaries(minb, ilen, dtype=F32, eps=True):
    """[I, 4], every operation rounded to dtype on its own: b0 = min_boundary, b_k = b_{k-1} + (max(len_{k-1}, 0) + 1e-4f)"""
    minb, ilen = np.asarray(minb, dtype=dtype), np.asarray(ilen, dtype=dtype)
    b = np.empty((len(minb), 4), dtype=dtype)
    b[:, 0] = minb
    for k in range(1, 4):
        cur = np.maximum(ilen[:, k - 1], dtype(0))
        if eps:
            cur = cur + dtype(EPS4)
        b[:, k] = b[:, k - 1] + cur
    return b


def _hv(d, ge=False):
    """[E, 5, 4]: H_ck = [s_ck d_k > 0]"""
    d = np.asarray(d)[:, None, :]
    lt = np.arange(4)[None, :] < np.arange(5)[:, None]
    return np.where(lt[None], d >= 0 if ge else d > 0, -d >= 0 if ge else -d > 0)


def _others(d):
    """[E, 5, 4]: prod over l != k of H_cl"""
    h = _hv(d)
    return np.stack([np.delete(h, k, axis=2).all(2) for k in range(4)], axis=2)


def st_cls_value(x, a, bd, dtype=F32, ge=False, mask=True):
    """from a and the entries' boundaries bd [E, 4], both in dtype: (cls int32, value dtype), the kernel's loop over the classes"""
    a, bd = np.asarray(a, dtype=dtype), np.asarray(bd, dtype=dtype)
    on = _hv(a[:, None] - bd, ge).all(2)                                    # [E, 5]
    cls = np.full(len(a), -1, dtype=np.int32)
    value = np.zeros(len(a), dtype=dtype)
    for c in range(5):
        cls = np.where(on[:, c], np.int32(c), cls)
        value = value + np.where(on[:, c], dtype(c + 1), dtype(0))
    return cls.astype(np.int32), np.where(np.asarray(x) > 0, value, dtype(0)).astype(dtype) if mask else value


# ---------------------------------------------------------------- generator forward
def st_norm(rowptr, x):
    x, n, K = f64(x), len(rowptr) - 1, np.diff(rowptr)
    root = np.sqrt(_seg(n, rows_of(rowptr), x * x))
    ref = np.maximum(root, EPS12)
    return ref, np.where(root > EPS12, (K / 2 + 2) * U * ref, 0.0)


def st_h1(rowptr, col, x, w1t, b1, norm):
    n, rows, K = len(rowptr) - 1, rows_of(rowptr), np.diff(rowptr)
    t = f64(x)[:, None] * f64(w1t)[col]
    nrm, b1 = f64(norm)[:, None], f64(b1)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):                   # a norm of 0 is the implementation's mistake: it fails, quietly
        ref = np.maximum(_seg(n, rows, t) / nrm + b1, 0.0)
        return ref, (K[:, None] + 4) * U * (_seg(n, rows, np.abs(t)) / nrm + np.abs(b1))


def st_a(rowptr, col, h1, w2, b2):
    t = f64(w2)[col] * f64(h1)[rows_of(rowptr)]
    bj = f64(b2)[col]
    z = t.sum(1) + bj
    dz = (HG + 8) * U * (np.abs(t).sum(1) + np.abs(bj))
    th = np.tanh(z)
    ref = 2.5 * th + 2.5
    slope = 1.0 - np.tanh(np.maximum(np.abs(z) - dz, 0.0)) ** 2
    return ref, 2.5 * slope * dz + (T + 2) * U * 2.5 * np.abs(th) + U * np.abs(ref)


# ---------------------------------------------------------------- generator backward, per row
def st_row_back(x, a, bd, mode, dvalue, scale):
    """{bbar [E, 4], zbar, eloss: (ref, bound)} from the entries' a and boundaries bd [E, 4]; scale as the kernel receives it"""
    x, a, bd = f64(x), f64(a), f64(bd)
    E = len(a)
    d = a[:, None] - bd
    if mode == 0:
        dv = np.where(x > 0, f64(dvalue), 0.0)
        gc = dv[:, None] * np.arange(1.0, 6.0)
        bgc = U * np.abs(gc)
        el = bel = np.zeros(E)
    else:
        dist = _hv(d).all(2).astype(np.float64)
        lse = np.log(np.exp(dist).sum(1))
        blse = (T + 4) * U + T * U * np.abs(lse)
        y = np.trunc(x).astype(np.int64) - 1
        use = (x > 0) & (y >= 0) & (y < 5)
        yc = np.clip(y, 0, 4)
        arg = dist - lse[:, None]
        p = np.exp(arg)
        bp = p * (blse[:, None] + U * np.abs(arg) + T * U)
        oh = (np.arange(5)[None, :] == yc[:, None]).astype(np.float64)
        gc = np.where(use[:, None], (p - oh) * scale, 0.0)
        bgc = np.where(use[:, None], scale * bp + 2 * U * np.abs(gc), 0.0)
        el = np.where(use, (lse - dist[np.arange(E), yc]) * scale, 0.0)
        bel = np.where(use, scale * blse + 2 * U * np.abs(el), 0.0)
    th = np.tanh(d)
    sech2 = 1.0 - th * th
    bs = 2 * np.abs(th) * (T * U * np.abs(th) + U * np.abs(d) * sech2) + U * th * th + U * sech2
    oth = _others(d)
    terms = oth * SGN[None] * gc[:, :, None] * sech2[:, None, :]                                       # [E, 5, 4]
    dd = terms.sum(1)
    bdd = (oth * (bgc[:, :, None] * sech2[:, None, :] + np.abs(gc)[:, :, None] * bs[:, None, :])).sum(1) + 6 * U * np.abs(terms).sum(1)
    abar = dd.sum(1)
    babar = bdd.sum(1) + 4 * U * np.abs(dd).sum(1)
    h2 = (a - 2.5) / 2.5
    q = 1.0 - h2 * h2
    bq = 5 * U * h2 * h2 + U * np.abs(q)
    zbar = abar * 2.5 * q
    return {"bbar": (-dd, bdd), "zbar": (zbar, 2.5 * (babar * np.abs(q) + np.abs(abar) * bq) + 3 * U * np.abs(zbar)), "eloss": (el, bel)}


def st_dpre(rowptr, col, zbar, w2, h1):
    n, rows, K = len(rowptr) - 1, rows_of(rowptr), np.diff(rowptr)
    t = f64(zbar)[:, None] * f64(w2)[col]
    gate = f64(h1) > 0
    return np.where(gate, _seg(n, rows, t), 0.0), np.where(gate, (K[:, None] + 2) * U * _seg(n, rows, np.abs(t)), 0.0)


# ---------------------------------------------------------------- generator backward, per item
def g_lists(I, rowptr, col):
    """the transposed list of rows rowptr[0 .. n] as the entry points take it: entries grouped by item, entry order kept inside an
    item; tent indexes col / x (absolute), trow is relative to rowptr"""
    e0, e1 = int(rowptr[0]), int(rowptr[-1])
    c = np.asarray(col[e0:e1], dtype=np.int64)
    order = np.argsort(c, kind="stable")
    tptr = np.zeros(I + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(c, minlength=I))
    return tptr, order + e0, rows_of(rowptr)[order]


def st_item(I, tptr, tent, trow, x, norm, h1, dpre, zbar):
    """{gw2, gw1t [I, 128]: (ref, bound)}; tent indexes x / zbar as given"""
    nj = np.diff(tptr)
    item = np.repeat(np.arange(I), nj)
    t2 = f64(zbar)[tent][:, None] * f64(h1)[trow]
    t1 = (f64(x)[tent] / f64(norm)[trow])[:, None] * f64(dpre)[trow]
    return {"gw2": (_seg(I, item, t2), (nj[:, None] + 2) * U * _seg(I, item, np.abs(t2))),
            "gw1t": (_seg(I, item, t1), (nj[:, None] + 3) * U * _seg(I, item, np.abs(t1)))}


# ---------------------------------------------------------------- discriminator
def st_d_h1(rowptr, col, val, w1t, b1):
    n, rows, K = len(rowptr) - 1, rows_of(rowptr), np.diff(rowptr)
    t = f64(val)[:, None] * f64(w1t)[col]
    b1 = f64(b1)[None, :]
    return np.maximum(_seg(n, rows, t) + b1, 0.0), (K[:, None] + 2) * U * (_seg(n, rows, np.abs(t)) + np.abs(b1))


def st_d_h2(h1, W2, b2):
    h1, W2, b2 = f64(h1), f64(W2), f64(b2)[None, :]
    return np.maximum(h1 @ W2.T + b2, 0.0), (HD1 + 8) * U * (np.abs(h1) @ np.abs(W2).T + np.abs(b2))


def st_d_p(h2, w3, b3):
    h2, w3, b3 = f64(h2), f64(w3), float(np.asarray(b3).reshape(-1)[0])
    s = h2 @ w3 + b3
    ds = (HD2 + 8) * U * (np.abs(h2) @ np.abs(w3) + abs(b3))
    sig = 1.0 / (1.0 + np.exp(-s))
    return sig, sig * (1.0 - sig) * np.exp(ds) * ds + (T + 2) * U * sig + TINY


def st_d_loss(p, y, n_side):
    """rowloss and dlogit (ref, bound) of the rows of one side (label y in {0, 1}, n_side rows) from p"""
    p = f64(p)
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
    l = -(y * lp + (1.0 - y) * lq)
    bl = T * U * np.abs(lp) if y == 1.0 else U + T * U * np.abs(lq)
    rl = l / n_side
    dl = (p - y) / np.maximum((1.0 - p) * p, EPS12) * (p * (1.0 - p)) / n_side
    return (rl, bl / n_side + 2 * U * np.abs(rl)), (dl, 10 * U * np.abs(dl))


def st_d_dz2(dlogit, h2, w3, dtype=F32):
    """bits: one product under the gate"""
    dlogit, h2, w3 = np.asarray(dlogit, dtype=dtype), np.asarray(h2, dtype=dtype), np.asarray(w3, dtype=dtype)
    return np.where(h2 > 0, dlogit[:, None] * w3[None, :], dtype(0)).astype(dtype)


def st_d_dz1(dz2, W2, h1):
    gate = f64(h1) > 0
    return np.where(gate, f64(dz2) @ f64(W2), 0.0), np.where(gate, (HD2 + 2) * U * (np.abs(f64(dz2)) @ np.abs(f64(W2))), 0.0)


def st_d_din(rows, col, w1t, dz1):
    """dL/dval at entries (row index into dz1, item)"""
    t = f64(w1t)[col] * f64(dz1)[rows]
    return t.sum(1), (HD1 + 8) * U * np.abs(t).sum(1)


def d_lists(I, nA, rpA, colA, nB, rpB, colB):
    """tptr, trow (0 .. nA + nB), tsrc (absolute index into valA / valB): all rows' entries grouped by item, A's rows first"""
    ka = np.arange(rpA[0], rpA[-1]) if nA else np.zeros(0, np.int64)
    kb = np.arange(rpB[0], rpB[-1]) if nB else np.zeros(0, np.int64)
    cols = np.concatenate([np.asarray(colA)[ka] if nA else ka, np.asarray(colB)[kb] if nB else kb]).astype(np.int64)
    rows = np.concatenate([rows_of(rpA) if nA else ka, nA + rows_of(rpB) if nB else kb])
    src = np.concatenate([ka, kb])
    order = np.argsort(cols, kind="stable")
    tptr = np.zeros(I + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(cols, minlength=I))
    return tptr, rows[order], src[order]


def st_d_grads(I, n, tptr, trow, tval, h1, dz1, h2, dz2, dlogit):
    """{W2, w3, w1t: (ref, bound)} and the bit-exact chains {b1, b2, b3} (float32); tval = the listed entries' values"""
    h1, dz1, h2, dz2, dl = f64(h1), f64(dz1), f64(h2), f64(dz2), f64(dlogit)
    nj = np.diff(tptr)
    item = np.repeat(np.arange(I), nj)
    t = f64(tval)[:, None] * dz1[trow]
    return {"W2": (dz2.T @ h1, (n + 2) * U * (np.abs(dz2).T @ np.abs(h1))), "w3": (dl @ h2, (n + 2) * U * (np.abs(dl) @ np.abs(h2))),
            "w1t": (_seg(I, item, t), (nj[:, None] + 2) * U * _seg(I, item, np.abs(t)))}


# ================================================================ the case
I = 300
LENGTHS = (0, 1, 2, 7, 8, 9, 0, 16, 17, 127, 128, 129, 257, 0)
SLICE = (2, 12)                # rows of the sliced calls: rowptr[2] = 1 > 0, and the 257-entry row and the last one stay outside
ABSENT = (0, 150, 151, 152, 299)
HOT = 7
ZERO_ROW = 5                   # its first two stored entries are 0.0 and -1.0
A_LENGTHS = (3, 0, 129, 1, 9, 257, 8, 0)
A_ROWS = (1, 8)                # D's A side: 7 rows of a CSR of 8, rowptrA[0] = 3
B_ROWS = (2, 14)               # D's B side: 12 rows of the generator's CSR, rowptrB[0] = 1
NA, NB = A_ROWS[1] - A_ROWS[0], B_ROWS[1] - B_ROWS[0]
B3_ONE, B3_ZERO = 40.0, -200.0  # b3 that saturate p to 1.0f and to 0.0f


def _csr(rng, lengths):
    pool = np.array([i for i in range(I) if i not in ABSENT and i != HOT])
    cols = []
    for L in lengths:
        c = rng.choice(pool, L - 1 if L >= 2 else L, replace=False)
        if L >= 2:
            c = np.concatenate([c, [HOT]])
            rng.shuffle(c)
        cols.append(c)
    rowptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lengths)
    col = np.concatenate(cols).astype(np.int32)
    return rowptr, col, rng.integers(1, 6, len(col)).astype(F32)


def _search_len(m):
    """fp32 search: a length L with fl(m + fl(max(L, 0) + 1e-4f)) == 2.5f"""
    L = F32(F32(2.5) - m) - EPS4
    for _ in range(64):
        b1 = F32(m + F32(max(L, F32(0)) + EPS4))
        if b1 == F32(2.5):
            return L
        L = np.nextafter(L, F32(1) if b1 < F32(2.5) else F32(-1))
    raise AssertionError("no fp32 length reaches 2.5f")


_CASE = None


def case():
    """the one case of the AushPlus stage tests (module constants above); computed once, never modified"""
    global _CASE
    if _CASE is not None:
        return _CASE
    rng = np.random.default_rng(20260)
    rowptr, col, x = _csr(rng, LENGTHS)
    x[rowptr[ZERO_ROW]], x[rowptr[ZERO_ROW] + 1] = 0.0, -1.0
    ka = int(rowptr[1])                                                    # the one entry of row 1
    kb = int(rowptr[2]) + int(col[rowptr[2]] == HOT)                       # the entry of row 2 that is not the hot item
    ja, jb = int(col[ka]), int(col[kb])
    assert ja != jb and HOT not in (ja, jb) and x[ka] > 0 and x[kb] > 0
    pad = np.arange(HG) >= HGR
    n32 = lambda *s, std: (std * rng.standard_normal(s)).astype(F32)       # noqa: E731
    gp = {"w1t": n32(I, HG, std=0.15), "b1": n32(HG, std=0.05), "w2": n32(I, HG, std=0.15), "b2": n32(I, std=0.03),
          "minb": (2.2 + 0.2 * rng.random(I)).astype(F32), "ilen": (0.12 * rng.random((I, 3)) - 0.01).astype(F32)}
    for k in ("w1t", "w2"):
        gp[k][:, pad] = 0
    gp["b1"][pad] = 0
    # exact boundaries: a == 2.5f for every entry of items ja and jb (tanhf(0) = 0); ja's b0 and jb's b1 are 2.5f
    for j in (ja, jb):
        gp["w2"][j], gp["b2"][j] = 0, 0
    gp["minb"][ja] = 2.5
    gp["minb"][jb] = 2.25
    gp["ilen"][jb, 0] = _search_len(F32(2.25))
    bd = boundaries(gp["minb"], gp["ilen"])
    assert bd[ja, 0] == F32(2.5) and bd[jb, 1] == F32(2.5) and bd[jb, 0] < F32(2.5) < bd[jb, 2]
    dp = {"w1t": n32(I, HD1, std=0.05), "b1": n32(HD1, std=0.02), "W2": n32(HD2, HD1, std=0.05), "b2": n32(HD2, std=0.02),
          "w3": n32(HD2, std=0.1), "b3": np.array([0.01], dtype=F32)}
    rpA, colA, valA = _csr(rng, A_LENGTHS)
    _CASE = {"rowptr": rowptr, "col": col, "x": x, "E": len(col), "n_rows": len(LENGTHS), "gp": gp, "dp": dp, "ka": ka, "kb": kb, "ja": ja,
             "jb": jb, "dvalue": rng.standard_normal(len(col)).astype(F32), "rpA": rpA, "colA": colA, "valA": valA}
    for v in list(_CASE.values()) + list(gp.values()) + list(dp.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _CASE


def pack_g(gp):
    return np.concatenate([gp[k].reshape(-1) for k in ("w1t", "b1", "w2", "b2", "minb", "ilen")]).astype(F32)


def unpack_g(flat):
    o = np.cumsum([0, I * HG, HG, I * HG, I, I, 3 * I])
    shp = {"w1t": (I, HG), "b1": (HG,), "w2": (I, HG), "b2": (I,), "minb": (I,), "ilen": (I, 3)}
    return {k: np.asarray(flat[o[i]:o[i + 1]]).reshape(shp[k]) for i, k in enumerate(shp)}


def pack_d(dp):
    return np.concatenate([dp[k].reshape(-1) for k in ("w1t", "b1", "W2", "b2", "w3", "b3")]).astype(F32)


def unpack_d(flat):
    o = np.cumsum([0, I * HD1, HD1, HD2 * HD1, HD2, HD2, 1])
    shp = {"w1t": (I, HD1), "b1": (HD1,), "W2": (HD2, HD1), "b2": (HD2,), "w3": (HD2,), "b3": (1,)}
    return {k: np.asarray(flat[o[i]:o[i + 1]]).reshape(shp[k]) for i, k in enumerate(shp)}


def g_view(c, rows=None):
    """the rows [r0, r1) of the case's CSR as a call sees them: rowptr keeps its absolute offsets into col / x"""
    r0, r1 = rows or (0, c["n_rows"])
    return {"rowptr": c["rowptr"][r0:r1 + 1], "col": c["col"], "x": c["x"], "n": r1 - r0, "cap_rows": c["n_rows"], "E": c["E"]}


def d_sides(c, nA=NA, nB=NB):
    return {"nA": nA, "rpA": c["rpA"][A_ROWS[0]:A_ROWS[0] + nA + 1], "colA": c["colA"], "valA": c["valA"], "nB": nB,
            "rpB": c["rowptr"][B_ROWS[0]:B_ROWS[0] + nB + 1], "colB": c["col"], "valB": c["x"], "cap": nA + nB}


# the calls the host and the GPU tests make: (rows, mode) of the generator, and rk_ap_d_step's forms
G_ROWS = {"whole": None, "slice": SLICE}
G_BACKWARD_RUNS = (("whole", 0), ("slice", 0), ("slice", 1), ("whole", 1))
_FULL = {"nA": NA, "nB": NB, "labelA": 1.0, "labelB": 0.0, "lists": True, "din": True, "b3": None}
D_RUNS = {"full": _FULL, "adversarial": dict(_FULL, nA=0, labelB=1.0), "nB0": dict(_FULL, nB=0), "no_dgrad": dict(_FULL, lists=False),
          "no_din": dict(_FULL, din=False), "p_one": dict(_FULL, b3=B3_ONE), "p_one_swapped": dict(_FULL, b3=B3_ONE, labelA=0.0, labelB=1.0),
          "p_zero": dict(_FULL, b3=B3_ZERO), "p_zero_swapped": dict(_FULL, b3=B3_ZERO, labelA=0.0, labelB=1.0)}


def d_params(c, run):
    return c["dp"] if run["b3"] is None else dict(c["dp"], b3=np.array([run["b3"]], dtype=F32))


def d_lists_of(s):
    return d_lists(I, s["nA"], s["rpA"], s["colA"], s["nB"], s["rpB"], s["colB"])


def scale_of(v):
    e0, e1 = v["rowptr"][0], v["rowptr"][-1]
    return F32(1.0) / F32(max(1, int((v["x"][e0:e1] > 0).sum())))


# ================================================================ a plain fp32 implementation (mut: one of MUTANTS or None)
def _sent(*shape, dtype=F32):
    return np.full(shape, SENTINEL, dtype=F32).view(dtype)


def g_forward_f32(v, gp, reverse=False, mut=None):
    rp, col, x, n = v["rowptr"], v["col"], v["x"], v["n"]
    out = {"norm": _sent(v["cap_rows"]), "h1": _sent(v["cap_rows"], HG), "a": _sent(v["E"]), "cls": _sent(v["E"], dtype=np.int32),
           "value": _sent(v["E"])}
    bd = boundaries(gp["minb"], gp["ilen"], eps=mut != "no_eps")
    with np.errstate(all="ignore"):
        for r in range(n):
            b, e = rp[r], rp[r + 1]
            xs, cs = x[b:e], col[b:e]
            nrm = np.sqrt(_dot(xs * xs, reverse))
            if mut != "norm_unclamped":
                nrm = np.maximum(nrm, F32(1e-12))
            h = np.maximum(_dot((xs[:, None] * gp["w1t"][cs]).T, reverse) / nrm + gp["b1"], F32(0))
            out["norm"][r], out["h1"][r] = nrm, h
            z = _dot(gp["w2"][cs] * h[None, :], reverse) + gp["b2"][cs]
            a = _r32(np.tanh(f64(z))) * F32(2.5) + F32(2.5)
            out["a"][b:e] = a
            out["cls"][b:e], out["value"][b:e] = st_cls_value(xs, a, bd[cs], ge=mut == "ge", mask=mut != "value_nomask")
    return out


def g_backward_f32(v, gp, fw, mode, dvalue, scale, lists, reverse=False, mut=None):
    """fw: the forward's buffers (norm, h1, a).  Returns zbar, bbar [E, 4], eloss, dpre, ggrad (packed) and loss [1]"""
    rp, col, x, n, E = v["rowptr"], v["col"], v["x"], v["n"], v["E"]
    out = {"zbar": _sent(E), "bbar": _sent(E, 4), "eloss": _sent(E), "dpre": _sent(v["cap_rows"], HG), "ggrad": _sent(I * (2 * HG + 5) + HG),
           "loss": _sent(1)}
    bd = boundaries(gp["minb"], gp["ilen"], eps=mut != "no_eps")
    scale = F32(scale)
    for r in range(n):
        b, e = int(rp[r]), int(rp[r + 1])
        ee = min(e, b + 128) if mut == "rowback_first128" else e
        a, xs = fw["a"][b:ee], x[b:ee]
        d = a[:, None] - bd[col[b:ee]]
        if mode == 0:
            dv = dvalue[b:ee] if mut == "dvalue_nomask" else np.where(xs > 0, dvalue[b:ee], F32(0))
            gc = (np.arange(1, 6, dtype=F32)[None, :] * dv[:, None]).astype(F32)
            el = np.zeros(ee - b, dtype=F32)
        else:
            dist = _hv(d).all(2).astype(F32)
            lse = _r32(np.log(f64(_dot(_r32(np.exp(f64(dist)))))))
            y = np.trunc(xs).astype(np.int64) - 1
            use = (xs > 0) & (y >= 0) & (y < 5)
            yc = np.clip(y, 0, 4)
            oh = (np.arange(5)[None, :] == yc[:, None]).astype(F32)
            gc = np.where(use[:, None], (_r32(np.exp(f64(dist - lse[:, None]))) - oh) * scale, F32(0)).astype(F32)
            el = np.where(use, (lse - dist[np.arange(ee - b), yc]) * scale, F32(0)).astype(F32)
        th = _r32(np.tanh(f64(d)))
        sech2 = F32(1) - th * th
        terms = np.where(_others(d), SGN.astype(F32)[None] * gc[:, :, None] * sech2[:, None, :], F32(0)).astype(F32)     # [e, 5, 4]
        dd = _dot(np.swapaxes(terms, 1, 2), reverse)
        abar = _dot(dd, reverse)
        h2 = (a - F32(2.5)) / F32(2.5)
        out["bbar"][b:ee], out["zbar"][b:ee], out["eloss"][b:ee] = -dd, abar * F32(2.5) * (F32(1) - h2 * h2), el
        acc = _dot((out["zbar"][b:e, None] * gp["w2"][col[b:e]]).T, reverse)
        out["dpre"][r] = np.where(fw["h1"][r] > 0, acc, F32(0))
    tptr, tent, trow = lists
    g = unpack_g(out["ggrad"])
    with np.errstate(all="ignore"):
        for j in range(I):
            k, r = tent[tptr[j]:tptr[j + 1]], trow[tptr[j]:tptr[j + 1]]
            g["w2"][j] = _dot((out["zbar"][k][:, None] * fw["h1"][r]).T, reverse)
            g["w1t"][j] = _dot(((x[k] / fw["norm"][r])[:, None] * out["dpre"][r]).T, reverse)
    g["b2"][:], g["minb"][:], g["ilen"][:] = side_sums(I, tptr, tent, out["zbar"], out["bbar"], gp["ilen"], gate=mut != "ilen_nogate")
    g["b1"][:] = colsum(out["dpre"][:n])
    if mode == 1:
        e0 = 0 if mut == "entry0_ignored" else int(rp[0])
        out["loss"][0] = sum_kernel(out["eloss"][e0:e0 + int(rp[-1] - rp[0])])
    return out


def d_step_f32(s, dp, labelA, labelB, lists=None, want_din=True, reverse=False, mut=None):
    """work arrays by name (rows >= nA + nB keep the sentinel), dgrad (packed, all sentinel without lists), dinB, loss [1]"""
    nA, nB = s["nA"], s["nB"]
    n = nA + nB
    out = {"h1": _sent(s["cap"], HD1), "dz1": _sent(s["cap"], HD1), "h2": _sent(s["cap"], HD2), "dz2": _sent(s["cap"], HD2), "p": _sent(s["cap"]),
           "dlogit": _sent(s["cap"]), "rowloss": _sent(s["cap"]), "dgrad": _sent(I * HD1 + HD1 + HD2 * HD1 + 2 * HD2 + 1), "dinB": _sent(len(s["valB"])),
           "loss": _sent(1)}
    with np.errstate(all="ignore"):
        for r in range(n):
            isA = r < nA
            rp, col, val, lr = (s["rpA"], s["colA"], s["valA"], r) if isA else (s["rpB"], s["colB"], s["valB"], r - nA)
            b, e = int(rp[lr]), int(rp[lr + 1])
            y = F32(labelA if isA else labelB)
            wgt = F32(1) / F32(n if mut == "bce_weight" else (nA if isA else nB))
            h1 = np.maximum(_dot((val[b:e, None] * dp["w1t"][col[b:e]]).T, reverse) + dp["b1"], F32(0))
            h2 = np.maximum(_dot(dp["W2"] * h1[None, :], reverse) + dp["b2"], F32(0))
            sl = _dot(dp["w3"] * h2, reverse) + dp["b3"][0]
            p = F32(1) / (F32(1) + _r32(np.exp(-f64(sl))))
            q = F32(1) - p
            l = -(y * np.maximum(_r32(np.log(f64(p))), F32(-100)) + (F32(1) - y) * np.maximum(_r32(np.log(f64(q))), F32(-100)))
            dl = F32((p - y) / np.maximum(q * p, F32(1e-12)) * (p * q) * wgt)
            dz2 = np.where(h2 > 0, dl * dp["w3"], F32(0)).astype(F32)
            dz1 = np.where(h1 > 0, _dot((dz2[:, None] * dp["W2"]).T, reverse), F32(0)).astype(F32)
            out["h1"][r], out["h2"][r], out["p"][r], out["rowloss"][r], out["dlogit"][r], out["dz2"][r], out["dz1"][r] = h1, h2, p, l * wgt, dl, dz2, dz1
            if not isA and want_din:
                ee = min(e, b + 8) if mut == "dinb_first8" else e
                out["dinB"][b:ee] = _dot(dp["w1t"][col[b:ee]] * dz1[None, :], reverse)
    out["loss"][0] = sum_kernel(out["rowloss"][:n])
    if lists is not None:
        tptr, trow, tsrc = lists
        g = unpack_d(out["dgrad"])
        tval = np.where(trow < nA, s["valA"][np.minimum(tsrc, len(s["valA"]) - 1)], s["valB"][np.minimum(tsrc, len(s["valB"]) - 1)]).astype(F32)
        g["W2"][:] = _dot(out["dz2"][:n].T[:, None, :] * out["h1"][:n].T[None, :, :], reverse)
        g["w3"][:] = _dot(out["dlogit"][:n][None, :] * out["h2"][:n].T, reverse)
        g["b2"][:], g["b1"][:], g["b3"][:] = colsum(out["dz2"][:n]), colsum(out["dz1"][:n]), colsum(out["dlogit"][:n, None])
        for j in range(I):
            q = slice(tptr[j], tptr[j + 1])
            g["w1t"][j] = _dot((tval[q][:, None] * out["dz1"][trow[q]]).T, reverse)
    return out


# ================================================================ a call's buffers against the stages
def _outside(arr, lo, hi):
    """0 when everything of arr outside [lo, hi) along axis 0 still holds the sentinel, else inf"""
    return 0.0 if all_sentinel(arr[:lo]) and all_sentinel(arr[hi:]) else INF


def check_g_forward(v, gp, o):
    rp, n = v["rowptr"], v["n"]
    e0, e1 = int(rp[0]), int(rp[-1])
    rl, col, x = rp - e0, v["col"][e0:e1], v["x"][e0:e1]
    cls, value = st_cls_value(x, o["a"][e0:e1], boundaries(gp["minb"], gp["ilen"])[col])
    r = {"norm": ratio(o["norm"][:n], *st_norm(rl, x)), "h1": ratio(o["h1"][:n], *st_h1(rl, col, x, gp["w1t"], gp["b1"], o["norm"][:n])),
         "a": ratio(o["a"][e0:e1], *st_a(rl, col, o["h1"][:n], gp["w2"], gp["b2"])), "cls": same_bits(o["cls"][e0:e1], cls),
         "value": same_bits(o["value"][e0:e1], value), "h1.pad+0": plus_zero(o["h1"][:n], np.arange(HG) >= HGR),
         "outside": max(_outside(o[k], e0, e1) for k in ("a", "cls", "value")) + max(_outside(o[k], 0, n) for k in ("norm", "h1"))}
    return r


def check_g_backward(v, gp, fw, o, mode, dvalue, scale, lists):
    rp, n = v["rowptr"], v["n"]
    e0, e1 = int(rp[0]), int(rp[-1])
    rl, col, x = rp - e0, v["col"][e0:e1], v["x"][e0:e1]
    bd = boundaries(gp["minb"], gp["ilen"])[col]
    rb = st_row_back(x, fw["a"][e0:e1], bd, mode, None if dvalue is None else dvalue[e0:e1], float(F32(scale)))
    zbar, bbar = o["zbar"][e0:e1], o["bbar"].reshape(-1, 4)[e0:e1]
    r = {"bbar": ratio(bbar, *rb["bbar"]), "zbar": ratio(zbar, *rb["zbar"]), "eloss": ratio(o["eloss"][e0:e1], *rb["eloss"]),
         "dpre": ratio(o["dpre"][:n], *st_dpre(rl, col, zbar, gp["w2"], fw["h1"][:n])), "dpre.gate+0": plus_zero(o["dpre"][:n], fw["h1"][:n] <= 0)}
    tptr, tent, trow = lists
    g = unpack_g(o["ggrad"])
    it = st_item(I, tptr, tent - e0, trow, x, fw["norm"][:n], fw["h1"][:n], o["dpre"][:n], zbar)
    gb2, gminb, gilen = side_sums(I, tptr, tent - e0, zbar, bbar, gp["ilen"])
    untouched, pad = np.diff(tptr) == 0, np.arange(HG) >= HGR
    r.update({"gw1t": ratio(g["w1t"], *it["gw1t"]), "gw2": ratio(g["w2"], *it["gw2"]), "gb1": same_bits(g["b1"], colsum(o["dpre"][:n])),
              "gb2": same_bits(g["b2"], gb2), "gminb": same_bits(g["minb"], gminb), "gilen": same_bits(g["ilen"], gilen),
              "untouched+0": max(plus_zero(g[k], untouched.reshape((-1,) + (1,) * (g[k].ndim - 1))) for k in ("w1t", "w2", "b2", "minb", "ilen")),
              "pad+0": max(plus_zero(g["w1t"], pad), plus_zero(g["w2"], pad), plus_zero(g["b1"], pad)),
              "outside": max(_outside(o[k].reshape(len(o["zbar"]), -1), e0, e1) for k in ("zbar", "bbar", "eloss")) + _outside(o["dpre"], 0, n)})
    r["loss"] = same_bits(o["loss"], np.array([sum_kernel(o["eloss"][e0:e1])], dtype=F32)) if mode == 1 else (0.0 if all_sentinel(o["loss"]) else INF)
    return r


def check_d_step(s, dp, o, labelA, labelB, lists=None, want_din=True):
    nA, nB = s["nA"], s["nB"]
    n = nA + nB
    ref, bnd = np.zeros((n, HD1)), np.zeros((n, HD1))
    if nA:
        ref[:nA], bnd[:nA] = st_d_h1(s["rpA"] - s["rpA"][0], s["colA"][s["rpA"][0]:s["rpA"][-1]], s["valA"][s["rpA"][0]:s["rpA"][-1]], dp["w1t"], dp["b1"])
    if nB:
        ref[nA:], bnd[nA:] = st_d_h1(s["rpB"] - s["rpB"][0], s["colB"][s["rpB"][0]:s["rpB"][-1]], s["valB"][s["rpB"][0]:s["rpB"][-1]], dp["w1t"], dp["b1"])
    h1, h2, p, dl, dz2, dz1 = (o[k][:n] for k in ("h1", "h2", "p", "dlogit", "dz2", "dz1"))
    r = {"h1": ratio(h1, ref, bnd), "h2": ratio(h2, *st_d_h2(h1, dp["W2"], dp["b2"])), "p": ratio(p, *st_d_p(h2, dp["w3"], dp["b3"]))}
    rl, rdl = [], []
    for lo, hi, y, cnt in ((0, nA, labelA, nA), (nA, n, labelB, nB)):
        if cnt:
            (a, ba), (b, bb) = st_d_loss(p[lo:hi], float(y), cnt)
            rl.append(ratio(o["rowloss"][lo:hi], a, ba))
            rdl.append(ratio(dl[lo:hi], b, bb))
    r.update({"rowloss": max(rl), "dlogit": max(rdl), "dz2": same_bits(dz2, st_d_dz2(dl, h2, dp["w3"])), "dz1": ratio(dz1, *st_d_dz1(dz2, dp["W2"], h1)),
              "dz1.gate+0": plus_zero(dz1, h1 <= 0), "loss": same_bits(o["loss"], np.array([sum_kernel(o["rowloss"][:n])], dtype=F32)),
              "finite": 0.0 if all(np.all(np.isfinite(o[k][:n])) for k in ("h1", "h2", "p", "dlogit", "dz2", "dz1", "rowloss")) and np.isfinite(o["loss"][0]) else INF,
              "outside": max(_outside(o[k], 0, n) for k in ("h1", "h2", "p", "dlogit", "dz2", "dz1", "rowloss"))})
    b0, b1 = (int(s["rpB"][0]), int(s["rpB"][-1])) if nB else (0, 0)
    if want_din and nB:
        r["dinB"] = ratio(o["dinB"][b0:b1], *st_d_din(nA + rows_of(s["rpB"]), s["colB"][b0:b1], dp["w1t"], dz1))
        r["dinB.outside"] = _outside(o["dinB"], b0, b1)
    else:
        r["dinB.outside"] = 0.0 if all_sentinel(o["dinB"]) else INF
    if lists is None:
        r["dgrad.outside"] = 0.0 if all_sentinel(o["dgrad"]) else INF
        return r
    tptr, trow, tsrc = lists
    tval = np.where(trow < nA, s["valA"][np.minimum(tsrc, len(s["valA"]) - 1)], s["valB"][np.minimum(tsrc, len(s["valB"]) - 1)])
    g = unpack_d(o["dgrad"])
    st = st_d_grads(I, n, tptr, trow, tval, h1, dz1, h2, dz2, dl)
    r.update({"gW2": ratio(g["W2"], *st["W2"]), "gw3": ratio(g["w3"], *st["w3"]), "gw1t": ratio(g["w1t"], *st["w1t"]),
              "gb2": same_bits(g["b2"], colsum(dz2)), "gb1": same_bits(g["b1"], colsum(dz1)), "gb3": same_bits(g["b3"], colsum(dl[:, None])),
              "untouched+0": plus_zero(g["w1t"], (np.diff(tptr) == 0)[:, None])})
    return r
