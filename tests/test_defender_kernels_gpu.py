"""GPU tests of the PCASelectUsers kernels one entry point at a time (csrc/pca.hip): each rk_pca_* call against a plain
fp64 numpy restatement of the same operation, at the shapes where the kernels' loops, tiles and key encodings change
behaviour.  Every output buffer is pre-filled with NaN (ints: a sentinel) and carries a sentinel margin after its end,
so an element the kernel skips, or one it writes past the end, fails the comparison."""
import os

import numpy as np
import pytest
import torch

from recad_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 64
SENTINEL = -777
U24, U52 = 2.0 ** -24, 2.0 ** -52
FLT_MIN = float(np.finfo(np.float32).tiny)


class Out:
    """A device buffer of n elements followed by MARGIN more, all NaN (floats) or SENTINEL (ints)."""

    def __init__(self, n, dtype, dev):
        self.n, self.fp = int(n), dtype.is_floating_point
        self.full = torch.full((self.n + MARGIN,), float("nan") if self.fp else SENTINEL, dtype=dtype, device=dev)
        self.t = self.full[: self.n]

    def host(self):
        """The n elements as numpy, after checking that the margin is as it was."""
        tail = self.full[self.n:].cpu().numpy()
        assert (np.isnan(tail).all() if self.fp else (tail == SENTINEL).all()), "the kernel wrote past the end of its output"
        return self.full[: self.n].cpu().numpy()

    def untouched(self):
        a = self.full.cpu().numpy()
        return bool(np.isnan(a).all() if self.fp else (a == SENTINEL).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _call():
    return _lib.lib(), _lib.ptr, _lib.stream_ptr


def _ulp(ref32):
    """Spacing of fp32 at |ref32| (at least the spacing at the smallest normal number)."""
    return np.spacing(np.maximum(np.abs(np.asarray(ref32, dtype=np.float32)), np.float32(FLT_MIN))).astype(np.float64)


def _csr(rows_cols, n_rows):
    """(rowptr int32, col int32, row-of-each-entry) from a list of per-row column arrays."""
    lens = np.array([len(c) for c in rows_cols], dtype=np.int64)
    assert len(rows_cols) == n_rows
    ptr = np.zeros(n_rows + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c in rows_cols]) if lens.sum() else np.zeros(0, dtype=np.int32)
    return ptr, col.astype(np.int32), np.repeat(np.arange(n_rows), lens)


# ---------------------------------------------------------------------------------------------------------- transpose
def _transpose_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("ncols"):
        n_cols, n_rows = int(name[5:]), 37
        rows = [np.sort(rng.choice(n_cols, size=min(n_cols, int(rng.integers(0, 21))), replace=False)) for _ in range(n_rows)]
        rows[3] = np.array([n_cols - 1])                     # the last column is used: the key's top bit below end_bit
        rows[5] = np.unique(np.array([0, n_cols - 1]))
    elif name == "empty":
        n_rows, n_cols = 50, 300
        live = np.setdiff1d(np.arange(n_cols), np.r_[0:4, 100:121, 290:300])
        rows = [np.sort(rng.choice(live, size=int(rng.integers(1, 30)), replace=False)) for _ in range(n_rows)]
        for r in (0, 1, 2, 20, 21, 22, 23, 24, 47, 48, 49):
            rows[r] = np.zeros(0, dtype=np.int64)
    elif name == "long_rows":
        n_rows, n_cols = 9, 5000
        rows = [np.sort(rng.choice(n_cols, size=s, replace=False)) for s in (3, 65, 0, 64 * 64 + 1, 64, 1, 100, 63, 2)]
    elif name == "nnz0":
        n_rows, n_cols = 5, 7
        rows = [np.zeros(0, dtype=np.int64)] * n_rows
    else:
        raise AssertionError(name)
    return n_rows, n_cols, rows


@pytest.mark.parametrize("name", ["ncols1", "ncols2", "ncols255", "ncols256", "ncols257", "ncols65536", "ncols65537", "empty",
                                  "long_rows", "nnz0"])
def test_transpose(gpu_device, name):
    n_rows, n_cols, rows = _transpose_case(name)
    ptr, col, row = _csr(rows, n_rows)
    nnz = len(col)
    rng = np.random.default_rng(5)
    val = (rng.permutation(nnz) + 1).astype(np.float32)      # all distinct and exact in fp32: a payload mix-up shows
    assert nnz < 2 ** 24 and len(np.unique(val)) == nnz
    d_ptr = _dev(ptr, gpu_device)
    d_col = _dev(col if nnz else np.zeros(1, dtype=np.int32), gpu_device)
    d_val = _dev(val if nnz else np.zeros(1, dtype=np.float32), gpu_device)
    # nnz == 0: the outputs still need an address (CovarianceOperator allocates max(nnz, 1) too); the margin provides it
    t_ptr, t_col, t_val = Out(n_cols + 1, torch.int32, gpu_device), Out(nnz, torch.int32, gpu_device), Out(nnz, torch.float32, gpu_device)
    L, P, S = _call()
    _lib.check(L.rk_pca_transpose(n_rows, n_cols, P(d_ptr), P(d_col), P(d_val), P(t_ptr.full), P(t_col.full), P(t_val.full),
                                  S(gpu_device)), "rk_pca_transpose")
    torch.cuda.synchronize()
    order = np.lexsort((row, col))
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int32)
    assert np.array_equal(t_ptr.host(), want_ptr)
    assert np.array_equal(t_col.host(), row[order].astype(np.int32))
    assert np.array_equal(t_val.host(), val[order])
    if nnz == 0:
        assert not t_ptr.host().any() and t_col.untouched() and t_val.untouched()


# ---------------------------------------------------------------------------------------------------------- col_scale
THRESH = np.float32(10.0) * np.finfo(np.float32).eps           # 1.25 * 2^-20, exact in fp32
# Allowed error of rk_pca_col_scale.  The kernel forms the variance in fp64 and rounds it once to fp32 (vf); the reference
# below does the same in another summation order, so the two fp64 values differ by about len * 2^-53 relative and vf can
# differ by one fp32 ulp only if the fp64 value lies that close to a rounding boundary: the columns here are checked to lie
# away from it (and from the threshold), so vf is the same number on both sides.  From vf on, the reference is fp64:
#   sigma = sqrtf(vf): HIP documents sqrtf to 1 ulp, i.e. at most 2^-23 relative             -> SIGMA_REL = 2^-23
#   inv   = 1.0f / sigma: sigma's error carries over relatively (2^-23), the fp32 division adds half an ulp (2^-24)
#                                                                                              -> INV_REL = 1.5 * 2^-23
# In ulps of the result that is at most 2 for sigma and 3 for inv_scale (an ulp is between 2^-24 and 2^-23 relative).
SIGMA_REL, INV_REL = 2.0 ** -23, 1.5 * 2.0 ** -23


def _var64(x, U):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    mean = x.sum() / U
    return (((x - mean) ** 2).sum() + (U - len(x)) * mean * mean) / U


def _scale_ref(columns, U):
    """(sigma, inv_scale) in fp64 from the fp32-rounded variance, and how far each fp64 variance is from the nearest
    point where its fp32 rounding would change (relative)."""
    sig, inv, slack = [], [], []
    for x in columns:
        v = _var64(x, U)
        vf = np.float32(v)
        lo, hi = float(np.nextafter(vf, np.float32(-np.inf))), float(np.nextafter(vf, np.float32(np.inf)))
        edge = min(abs(v - 0.5 * (lo + float(vf))), abs(v - 0.5 * (hi + float(vf)))) / max(abs(v), 1e-300) if v > 0 else 1.0
        slack.append(edge)
        if not vf >= THRESH:
            vf = np.float32(1.0)
        sig.append(np.sqrt(np.float64(vf)))
        inv.append(1.0 / np.sqrt(np.float64(vf)))
    return np.array(sig), np.array(inv), np.array(slack)


def _run_col_scale(columns, U, dev, with_sigma=True):
    ptr = np.zeros(len(columns) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(c) for c in columns])
    val = np.concatenate([np.asarray(c, dtype=np.float32) for c in columns] + [np.zeros(1, dtype=np.float32)])
    inv, sig = Out(len(columns), torch.float32, dev), Out(len(columns), torch.float32, dev)
    d_ptr, d_val = _dev(ptr, dev), _dev(val, dev)        # named: the inputs must outlive the launch
    L, P, S = _call()
    _lib.check(L.rk_pca_col_scale(len(columns), U, P(d_ptr), P(d_val), P(inv.t), P(sig.t) if with_sigma else None, S(dev)),
               "rk_pca_col_scale")
    torch.cuda.synchronize()
    return inv, sig


def _threshold_column(target, U=4096):
    """n copies of one fp32 value x among U users whose variance x^2 n (U - n) / U^2 rounds to the fp32 number `target`, well
    inside its rounding interval."""
    target = np.float32(target)
    for n in range(1, U):
        x0 = np.float32(np.sqrt(float(target) * U * U / (n * (U - n))))
        for step in range(-3, 4):
            x = x0
            for _ in range(abs(step)):
                x = np.nextafter(x, np.float32(np.inf if step > 0 else -np.inf))
            v = float(x) * float(x) * n * (U - n) / (U * U)
            if np.float32(v) == target and abs(v - float(target)) < 0.25 * float(np.spacing(target)):
                col = np.full(n, x, dtype=np.float32)
                v2 = _var64(col, U)
                if np.float32(v2) == target and abs(v2 - float(target)) < 0.3 * float(np.spacing(target)):
                    return col
    raise AssertionError(f"no column with fp32 variance {target!r}")


def test_col_scale_random_columns(gpu_device):
    rng = np.random.default_rng(11)
    U = 300
    cols = []
    for n in (0, 1, 63, 64, 65, 200, 0, 7, 128, 129, 300):
        cols.append(rng.integers(1, 6, n).astype(np.float32))                        # ratings 1..5
        cols.append((rng.standard_normal(n) * 2.5).astype(np.float32))               # negative and fractional
    cols.append(np.full(U, 4.0, dtype=np.float32))                                   # every user, one value: variance exactly 0
    cols.append(np.full(U, -2.5, dtype=np.float32))
    cols.append(np.zeros(0, dtype=np.float32))                                       # the last column empty
    sig_ref, inv_ref, slack = _scale_ref(cols, U)
    v = np.array([_var64(c, U) for c in cols])
    live = v > 0
    # the reference's own fp64-vs-fp32 rounding cannot flip a case: away from the threshold by 1e-3 relative, and away from an
    # fp32 rounding boundary by far more than fp64 summation order moves the variance (len * 2^-53 < 1e-13)
    assert np.all(np.abs(v[live] / float(THRESH) - 1.0) > 1e-3) and np.all(slack[live] > 1e-11), (v, slack)
    assert _var64(cols[-3], U) == 0.0 and _var64(cols[-2], U) == 0.0
    inv, sig = _run_col_scale(cols, U, gpu_device)
    got_inv, got_sig = inv.host().astype(np.float64), sig.host().astype(np.float64)
    print("col_scale: max rel err sigma %.3g inv %.3g" % (np.abs(got_sig / sig_ref - 1).max(), np.abs(got_inv / inv_ref - 1).max()))
    assert np.all(np.abs(got_sig - sig_ref) <= SIGMA_REL * sig_ref), (got_sig, sig_ref)
    assert np.all(np.abs(got_inv - inv_ref) <= INV_REL * inv_ref), (got_inv, inv_ref)
    for j in (0, 1, 12, 13, len(cols) - 3, len(cols) - 2, len(cols) - 1):               # empty and constant columns: scale exactly 1
        assert got_inv[j] == 1.0 and got_sig[j] == 1.0, j
    inv2, _ = _run_col_scale(cols, U, gpu_device, with_sigma=False)                  # sigma is optional
    assert np.array_equal(inv2.host(), inv.host())


def test_col_scale_threshold(gpu_device):
    """var < 10 * FLT_EPSILON, decided on the fp32-rounded variance (not on its square root), counts as constant."""
    below, above = np.nextafter(THRESH, np.float32(0)), np.nextafter(THRESH, np.float32(1))
    cols = [_threshold_column(t) for t in (below, THRESH, above)]
    inv, sig = _run_col_scale(cols, 4096, gpu_device)
    got_inv, got_sig = inv.host().astype(np.float64), sig.host().astype(np.float64)
    assert got_inv[0] == 1.0 and got_sig[0] == 1.0, "one ulp below the threshold: constant"
    for j, t in ((1, THRESH), (2, above)):
        s = np.sqrt(np.float64(t))
        assert abs(got_sig[j] - s) <= SIGMA_REL * s and abs(got_inv[j] - 1 / s) <= INV_REL / s, (j, got_sig[j], s)
    # a million users: one rating of 1.0 has variance (1 - 1e-6) * 1e-6 < 1.19e-6 (constant, scale 1), two have 2e-6 (not)
    U = 10 ** 6
    cols = [np.ones(1, dtype=np.float32), np.ones(2, dtype=np.float32), np.full(1, 5.0, dtype=np.float32)]
    assert np.float32(_var64(cols[0], U)) < THRESH < np.float32(_var64(cols[1], U))
    sig_ref, inv_ref, _ = _scale_ref(cols, U)
    inv, sig = _run_col_scale(cols, U, gpu_device)
    got_inv, got_sig = inv.host().astype(np.float64), sig.host().astype(np.float64)
    assert got_inv[0] == 1.0 and got_sig[0] == 1.0 and inv_ref[0] == 1.0
    assert np.all(np.abs(got_sig - sig_ref) <= SIGMA_REL * sig_ref) and np.all(np.abs(got_inv - inv_ref) <= INV_REL * inv_ref)
    assert got_inv[1] > 700.0 and got_inv[2] > 190.0        # sqrt(1 / 2e-6) = 707, sqrt(1 / 25e-6) = 200


def test_col_scale_is_sklearns_rule(gpu_device):
    """transpose + col_scale on the small matrix that make_golden_pca.py ran through sklearn.preprocessing.scale(csr, axis=0,
    with_mean=False): constant and near-constant columns included, the scaled values as sklearn returned them."""
    g = np.load(os.path.join(GOLDEN, "pca_sklearn_scale.npz"))
    U, I, nnz = int(g["n_users"]), int(g["n_items"]), len(g["idx"])
    d_ptr, d_col, d_val = _dev(g["ptr"], gpu_device), _dev(g["idx"], gpu_device), _dev(g["val"], gpu_device)
    t_ptr, t_col, t_val = Out(I + 1, torch.int32, gpu_device), Out(nnz, torch.int32, gpu_device), Out(nnz, torch.float32, gpu_device)
    inv = Out(I, torch.float32, gpu_device)
    L, P, S = _call()
    _lib.check(L.rk_pca_transpose(U, I, P(d_ptr), P(d_col), P(d_val), P(t_ptr.t), P(t_col.t), P(t_val.t), S(gpu_device)), "rk_pca_transpose")
    _lib.check(L.rk_pca_col_scale(I, U, P(t_ptr.t), P(t_val.t), P(inv.t), None, S(gpu_device)), "rk_pca_col_scale")
    torch.cuda.synchronize()
    got = g["val"].astype(np.float64) * inv.host().astype(np.float64)[g["idx"]]
    want = g["scaled"].astype(np.float64)
    # sklearn multiplies in fp32 by 1 / sqrt(var) formed in fp32: its own roundings (sqrt, division, product: half an ulp each)
    # add 1.5 * 2^-23 to INV_REL
    assert np.all(np.abs(got - want) <= (INV_REL + 1.5 * 2.0 ** -23) * np.abs(want)), np.abs(got / want - 1).max()
    unit = np.isin(g["idx"], g["unit_columns"])
    assert unit.any() and np.array_equal(got[unit], g["val"][unit].astype(np.float64)), "sklearn left these columns unscaled"


# --------------------------------------------------------------------------------------------------------------- spmm
def _spmm_problem(b, rng):
    npw = 64 // (b // 4)
    lens = [0, 1, npw - 1, npw, npw + 1, 4 * npw - 1, 4 * npw, 4 * npw + 1, 3001, 2, 0, 8 * npw + 3, 5, 0]
    lens += [int(x) for x in rng.integers(0, 3 * npw, 7)]
    n_rows, n_cols = len(lens), 1500
    assert n_rows % 4 != 0
    rows = []
    for n in lens:
        c = rng.integers(0, n_cols, n)
        if n >= 2:
            c[1] = c[0]                                     # a duplicate column id inside the row
        if n >= 3:
            c[2] = n_cols - 1
        rows.append(c)
    ptr, col, row = _csr(rows, n_rows)
    val = (rng.standard_normal(len(col)) * 2).astype(np.float32)
    c_in = (rng.standard_normal(n_cols) + 0.5).astype(np.float32)
    r_out = (rng.standard_normal(n_rows) - 0.5).astype(np.float32)
    X = rng.standard_normal((n_cols, b)).astype(np.float32)
    return n_rows, n_cols, ptr, col, row, val, c_in, r_out, X


@pytest.mark.parametrize("r_out_on", [False, True])
@pytest.mark.parametrize("c_in_on", [False, True])
@pytest.mark.parametrize("b", [8, 16])
def test_spmm(gpu_device, b, c_in_on, r_out_on):
    rng = np.random.default_rng(100 + b)
    n_rows, n_cols, ptr, col, row, val, c_in, r_out, X = _spmm_problem(b, rng)
    Y = Out(n_rows * b, torch.float32, gpu_device)
    L, P, S = _call()
    d = [_dev(a, gpu_device) for a in (ptr, col, val, c_in, r_out, X)]
    _lib.check(L.rk_pca_spmm(n_rows, P(d[0]), P(d[1]), P(d[2]), P(d[3]) if c_in_on else None, P(d[4]) if r_out_on else None, b,
                             P(d[5]), P(Y.t), S(gpu_device)), "rk_pca_spmm")
    torch.cuda.synchronize()
    got = Y.host().astype(np.float64).reshape(n_rows, b)
    w = val.astype(np.float64) * (c_in.astype(np.float64)[col] if c_in_on else 1.0)
    terms = w[:, None] * X.astype(np.float64)[col]                                        # [nnz, b]
    ref, mag = np.zeros((n_rows, b)), np.zeros((n_rows, b))
    np.add.at(ref, row, terms)
    np.add.at(mag, row, np.abs(terms))
    r = r_out.astype(np.float64)[:, None] if r_out_on else 1.0
    ref, mag = ref * r, mag * np.abs(r)
    lens = np.diff(ptr).astype(np.float64)[:, None]
    bound = (lens + 4) * U24 * mag
    err = np.abs(got - ref)
    print("spmm b=%d cin=%d rout=%d: max err / bound %.3g" % (b, c_in_on, r_out_on, (err / np.maximum(bound, 1e-300))[mag > 0].max()))
    assert not np.isnan(got).any(), "a row was skipped"
    assert np.all(err <= bound), (np.argwhere(err > bound)[:5], err.max())
    assert np.all(got[np.diff(ptr) == 0] == 0.0)


@pytest.mark.parametrize("b", [8, 16])
def test_spmm_refusals_write_nothing(gpu_device, b):
    rng = np.random.default_rng(7)
    n_rows, n_cols, ptr, col, row, val, c_in, r_out, X = _spmm_problem(b, rng)
    L, P, S = _call()
    d_ptr, d_col, d_val = (_dev(a, gpu_device) for a in (ptr, col, val))
    Xp = torch.zeros(n_cols * 16 + 4, dtype=torch.float32, device=gpu_device)
    Y = Out(n_rows * 16, torch.float32, gpu_device)
    assert Xp.data_ptr() % 16 == 0 and Y.t.data_ptr() % 16 == 0
    cases = {"width 12": (12, P(Xp[: n_cols * 16]), P(Y.t)), "null X": (b, None, P(Y.t)), "null Y": (b, P(Xp[: n_cols * 16]), None),
             "X off the 16-byte grid": (b, P(Xp[1: n_cols * 16 + 1]), P(Y.t)), "Y off the grid": (b, P(Xp[: n_cols * 16]), P(Y.full[1:]))}
    for what, (width, x, y) in cases.items():
        rc = L.rk_pca_spmm(n_rows, P(d_ptr), P(d_col), P(d_val), None, None, width, x, y, S(gpu_device))
        assert rc != 0, what
        with pytest.raises(_lib.HipCallError, match="rk_pca_spmm"):
            _lib.check(rc, "rk_pca_spmm")
        torch.cuda.synchronize()
        assert Y.untouched(), what


# ------------------------------------------------------------------------------------------------------------ sq_spmv
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_sq_spmv(gpu_device, k, pad):
    rng = np.random.default_rng(200 + k)
    n_cols, ldv = 777, k + pad
    lens = [0, 1, 63, 64, 65, 0, 300, 2, 0] + [int(x) for x in rng.integers(0, 150, 12)] + [0]
    n_rows = len(lens)
    rows = [rng.choice(n_cols, n, replace=False) for n in lens]
    ptr, col, row = _csr(rows, n_rows)
    val = np.where(rng.random(len(col)) < 0.5, rng.integers(-5, 6, len(col)), rng.standard_normal(len(col)) * 3).astype(np.float32)
    V = np.full((n_cols, ldv), np.nan, dtype=np.float32)
    V[:, :k] = rng.standard_normal((n_cols, k)).astype(np.float32) * 0.05
    w, dist = Out(n_cols, torch.float32, gpu_device), Out(n_rows, torch.float32, gpu_device)
    L, P, S = _call()
    d = [_dev(a, gpu_device) for a in (ptr, col, val, V)]
    _lib.check(L.rk_pca_sq_spmv(n_rows, n_cols, P(d[0]), P(d[1]), P(d[2]), P(d[3]), ldv, k, P(w.t), P(dist.t), S(gpu_device)), "rk_pca_sq_spmv")
    torch.cuda.synchronize()
    w64 = V[:, :k].astype(np.float64).sum(axis=1)
    w_ref = w64.astype(np.float32)
    got_w = w.host()
    assert not np.isnan(got_w).any(), "columns beyond k were read into w, or a row of w was skipped"
    assert np.all(np.abs(got_w.astype(np.float64) - w_ref.astype(np.float64)) <= _ulp(w_ref) + k * U52 * np.abs(V[:, :k]).sum(1))
    # dist in fp64 from the reference's w; where the kernel's w sits on the other side of a rounding (within the ulp just
    # checked) that difference times the squared ratings is added to the bound
    a2 = val.astype(np.float64) ** 2
    ref, mag, dw = np.zeros(n_rows), np.zeros(n_rows), np.zeros(n_rows)
    np.add.at(ref, row, a2 * w_ref.astype(np.float64)[col])
    np.add.at(mag, row, a2 * np.abs(w_ref.astype(np.float64))[col])
    np.add.at(dw, row, a2 * np.abs(got_w.astype(np.float64) - w_ref.astype(np.float64))[col])
    got = dist.host()
    assert not np.isnan(got).any()
    ref32 = ref.astype(np.float32)
    bound = _ulp(ref32) + (np.diff(ptr) + 1) * U52 * mag + dw     # one fp32 rounding, plus fp64 accumulation in another order
    assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= bound), np.abs(got - ref32).max()
    assert np.all(got[np.diff(ptr) == 0] == 0.0) and (got < 0).any(), "the sum of eigenvectors gives negative distances too"
    if k > 1:
        rc = L.rk_pca_sq_spmv(n_rows, n_cols, P(d[0]), P(d[1]), P(d[2]), P(d[3]), k - 1, k, P(w.t), P(dist.t), S(gpu_device))
        assert rc != 0, "ldv < k must be refused"


# --------------------------------------------------------------------------------------------------------------- gram
GRAM_N = [1, 63, 64, 65, 255, 256, 257, 256 * 64 + 1, 100003]


def _gram(dev, Pm, Qm):
    n, p, q = Pm.shape[0], Pm.shape[1], (0 if Qm is None else Qm.shape[1])
    ww = (p + q) ** 2
    part = torch.full((_lib.RK_PCA_GRAM_BLOCKS * 32 * 32,), float("nan"), dtype=torch.float64, device=dev)
    G = Out(ww, torch.float64, dev)
    L, P, S = _call()
    _lib.check(L.rk_pca_gram(n, P(Pm), p, P(Qm), q, P(part), P(G.t), S(dev)), "rk_pca_gram")
    torch.cuda.synchronize()
    used = _lib.RK_PCA_GRAM_BLOCKS * ww
    assert bool(torch.isnan(part[used:]).all()), "partial sums written past blocks * (p + q)^2"
    return G.host().reshape(p + q, p + q)


@pytest.mark.parametrize("pq", [(8, 0), (8, 8), (16, 0), (16, 16), (3, 0), (5, 7), (1, 0)])
def test_gram(gpu_device, pq):
    p, q = pq
    rng = np.random.default_rng(300 + 32 * p + q)
    for n in GRAM_N:
        Z = rng.standard_normal((n, p + q)).astype(np.float32)
        Z[rng.random(n) < 0.1] *= 100.0                                  # uneven row norms
        Pm = _dev(Z[:, :p], gpu_device)
        Qm = _dev(Z[:, p:], gpu_device) if q else None
        G = _gram(gpu_device, Pm, Qm)
        Z64 = Z.astype(np.float64)
        ref, bound = Z64.T @ Z64, n * U52 * (np.abs(Z64).T @ np.abs(Z64))
        assert not np.isnan(G).any(), (n, "an element of G was skipped")
        assert np.all(np.abs(G - ref) <= bound), (n, np.abs(G - ref).max(), bound.min())
        assert np.array_equal(G, G.T), (n, "G[i, j] and G[j, i] are the same products in the same order")
        assert np.array_equal(G, _gram(gpu_device, Pm, Qm)), (n, "two runs differ")


def test_gram_refusals(gpu_device):
    Z = torch.ones(10, 33, dtype=torch.float32, device=gpu_device)
    Q = torch.ones(10, 16, dtype=torch.float32, device=gpu_device)
    part = torch.zeros(_lib.RK_PCA_GRAM_BLOCKS * 32 * 32, dtype=torch.float64, device=gpu_device)
    G = Out(33 * 33, torch.float64, gpu_device)
    L, P, S = _call()
    for args in ((10, P(Z), 17, P(Q), 16), (10, P(Z), 33, None, 0), (10, P(Q), 16, None, 16), (0, P(Q), 16, None, 0)):
        rc = L.rk_pca_gram(*args, P(part), P(G.t), S(gpu_device))
        with pytest.raises(_lib.HipCallError, match="rk_pca_gram"):
            _lib.check(rc, "rk_pca_gram")
    torch.cuda.synchronize()
    assert G.untouched()


# ------------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("pq", [(8, 8), (8, 3), (16, 16), (16, 10), (32, 32), (1, 1)])
def test_update(gpu_device, pq):
    p, q = pq
    rng = np.random.default_rng(400 + 32 * p + q)
    L, P, S = _call()
    for n in GRAM_N:
        V = rng.standard_normal((n, p)).astype(np.float32)
        M = rng.standard_normal((p, q)) * np.exp(rng.standard_normal((p, q)) * 3)       # fp64, wide range: 1 / lambda scalings
        out = Out(n * q, torch.float32, gpu_device)
        d_V, d_M = _dev(V, gpu_device), _dev(M, gpu_device)
        _lib.check(L.rk_pca_update(n, P(d_V), p, P(d_M), q, P(out.t), S(gpu_device)), "rk_pca_update")
        torch.cuda.synchronize()
        got = out.host().reshape(n, q)
        V64 = V.astype(np.float64)
        ref32 = (V64 @ M).astype(np.float32)
        bound = _ulp(ref32) + (p + 1) * U52 * (np.abs(V64) @ np.abs(M))       # one fp32 rounding of an fp64 sum of p products
        assert not np.isnan(got).any(), (n, "an element was skipped")
        assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= bound), (n, np.abs(got - ref32).max())
        if n == 65:
            rc = L.rk_pca_update(n, P(d_V), p, P(d_M), min(q, p), P(d_V), S(gpu_device))
            with pytest.raises(_lib.HipCallError, match="rk_pca_update"):
                _lib.check(rc, "rk_pca_update")
            torch.cuda.synchronize()
            assert np.array_equal(d_V.cpu().numpy(), V), "V == out is refused, V stays as it was"


# ------------------------------------------------------------------------------------------------------------- select
DENORM = np.array([1, 2, 0x7FFFFF], dtype=np.uint32).view(np.float32)     # the smallest, the next, the largest denormal
FLT_MAX = np.finfo(np.float32).max


def _select_input(kind, n, rng):
    if kind == "all_equal":
        return np.full(n, 3.5, dtype=np.float32)
    if kind == "two_values":
        return rng.choice(np.array([1.0, -2.0], dtype=np.float32), n)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0], dtype=np.float32), n)
    if kind == "signed":
        return (rng.standard_normal(n) * 1e-3).astype(np.float32)
    if kind == "ties":
        return rng.choice(np.array([-3.0, -0.0, 0.0, 2.0, -1e-3, 1e-3, 7.0], dtype=np.float32), n)
    if kind == "denormals":
        pool = np.concatenate([DENORM, -DENORM, np.array([0.0, -0.0, FLT_MIN, -FLT_MIN], dtype=np.float32)])
        return rng.choice(pool, n)
    if kind == "flt_max":
        d = rng.standard_normal(n).astype(np.float32)
        d[rng.random(n) < 0.3] = FLT_MAX
        d[rng.random(n) < 0.3] = -FLT_MAX
        return d
    raise AssertionError(kind)


def _select(dist, m, dev):
    n = len(dist)
    order, d_dist = Out(m, torch.int32, dev), _dev(dist, dev)
    L, P, S = _call()
    _lib.check(L.rk_pca_select(n, P(d_dist), m, P(order.full), S(dev)), "rk_pca_select")
    torch.cuda.synchronize()
    return order.host()            # order[m:] (the margin) must still hold the sentinel


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
@pytest.mark.parametrize("kind", ["all_equal", "two_values", "zeros", "signed", "ties", "denormals", "flt_max"])
def test_select(gpu_device, kind, n):
    rng = np.random.default_rng(500 + n)
    dist = _select_input(kind, n, rng)
    folded = np.where(dist == 0, np.float32(0.0), dist)        # Python compares -0.0 == 0.0: one key, the lower id first
    assert not np.signbit(folded[folded == 0]).any()
    want = np.argsort(folded, kind="stable")
    if kind == "denormals" and n > 1:
        assert (np.abs(dist[dist != 0]) < FLT_MIN).any()
    for m in sorted({0, 1, n // 2, n}):
        got = _select(dist, m, gpu_device)
        assert np.array_equal(got, want[:m].astype(np.int32)), (m, got[:10], want[:10], dist[want[:10]])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_select_refuses_non_finite(gpu_device, bad):
    rng = np.random.default_rng(9)
    dist = rng.standard_normal(1000).astype(np.float32)
    dist[137] = bad
    with pytest.raises(_lib.HipCallError, match=r"rk_pca_select.* 1 non-finite"):
        _select(dist, 10, gpu_device)
    dist[[0, 999]] = bad
    with pytest.raises(_lib.HipCallError, match=r"rk_pca_select.* 3 non-finite"):
        _select(dist, 1000, gpu_device)
