"""GPU tests of the KnnSelectUsers kernels one entry point at a time (csrc/knn.hip) against the numpy restatement of the
definition (tests/_knn_restate.py).  topw and degsim are compared bit for bit: no tolerance, no excluded case.  Every output
buffer is pre-filled with NaN (ints: a sentinel) and carries a 64-element margin that must stay as it was."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _knn_restate as R

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 64, -777


class Out:
    """A device buffer of n elements followed by MARGIN more, all NaN (floats) or SENTINEL (ints)."""

    def __init__(self, n, dtype, dev):
        self.n, self.fp = int(n), dtype.is_floating_point
        self.full = torch.full((self.n + MARGIN,), float("nan") if self.fp else SENTINEL, dtype=dtype, device=dev)

    def host(self):
        tail = self.full[self.n:].cpu().numpy()
        assert (np.isnan(tail).all() if self.fp else (tail == SENTINEL).all()), "the kernel wrote past the end of its output"
        return self.full[: self.n].cpu().numpy()

    def untouched(self):
        a = self.full.cpu().numpy()
        return bool(np.isnan(a).all() if self.fp else (a == SENTINEL).all())


def _dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(dev)     # an empty array still needs an address


def _csr(rows, vals=None):
    """(ptr int32, idx int32, val float32) from per-row column lists (sorted here) and optional per-row value lists."""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    order = [np.argsort(np.asarray(r, dtype=np.int64), kind="stable") for r in rows]
    idx = np.concatenate([np.asarray(r, dtype=np.int32)[o] for r, o in zip(rows, order)] + [np.zeros(0, dtype=np.int32)])
    if vals is None:
        val = np.ones(len(idx), dtype=np.float32)
    else:
        val = np.concatenate([np.asarray(v, dtype=np.float32)[o] for v, o in zip(vals, order)] + [np.zeros(0, dtype=np.float32)])
    return ptr, idx.astype(np.int32), val.astype(np.float32)


def _transpose(ptr, idx, val, n_items):
    """The transposed CSR rk_pca_transpose produces: users ascending inside a column."""
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    o = np.lexsort((row, idx))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_items))]).astype(np.int32)
    return colptr, row[o].astype(np.int32), val[o].astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- rk_knn_norms
def _norms(dev, ptr, idx, val, n_items):
    U = len(ptr) - 1
    rn, st = Out(U, torch.float32, dev), Out(2, torch.int32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, dev) for a in (ptr, idx, val)]       # held until the call has returned
    rc = L.rk_knn_norms(U, n_items, P(d[0]), P(d[1]), P(d[2]), P(rn.full), P(st.full), S(dev))
    torch.cuda.synchronize()
    return rc, rn, st


def _norm_rows(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    I = 300
    rows = [np.sort(rng.choice(I, size=int(n), replace=False)) for n in rng.integers(1, 90, size=70)]
    rows[0], rows[7], rows[69] = np.zeros(0, dtype=np.int64), np.array([I - 1]), np.zeros(0, dtype=np.int64)    # empty rows, a row of 1
    rows[9] = np.arange(200)                     # more than three lane strides
    if name == "implicit":
        vals = [np.ones(len(r)) for r in rows]
    else:
        vals = [rng.integers(1, 6, size=len(r)).astype(np.float64) for r in rows]
        if name == "value127":
            vals[3][:] = 127
            vals[9][::3] = 127
    return rows, vals, I


@pytest.mark.parametrize("name", ["implicit", "ratings", "value127"])
def test_norms(gpu_device, name):
    rows, vals, I = _norm_rows(name)
    ptr, idx, val = _csr(rows, vals)
    assert R.first_violation(ptr, idx, val, I) is None
    rc, rn, st = _norms(gpu_device, ptr, idx, val, I)
    assert rc == 0 and st.host().tolist() == [0, -1]
    want = R.rnorm(R.dense(ptr, idx, val, I))
    assert want[0] == 0 and want[7] in (np.float32(1), np.float32(1 / 5), np.float32(1 / 4), np.float32(1 / 3), np.float32(1 / 2))
    assert np.array_equal(rn.host().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name,rule", [("value0", 1), ("value128", 1), ("value2.5", 1), ("value-1", 1), ("valuenan", 1),
                                       ("duplicate", 2), ("descending", 2), ("col_n_items", 2), ("col_negative", 2),
                                       ("two_rows", 2), ("same_rule_twice", 2), ("both_rules", 1)])
def test_norms_refusals(gpu_device, name, rule):
    rows, vals, I = _norm_rows("ratings")
    ptr, idx, val = _csr(rows, vals)
    row = 37
    b = int(ptr[row]) + 5
    assert ptr[row + 1] - ptr[row] > 8
    if name.startswith("value"):
        val[b] = float(name[5:])
    elif name == "duplicate":
        idx[b + 1] = idx[b]
    elif name == "descending":
        idx[b], idx[b + 1] = idx[b + 1], idx[b]
    elif name == "col_n_items":
        idx[ptr[row + 1] - 1] = I
    elif name == "col_negative":
        idx[ptr[row]] = -1
    elif name == "two_rows":                       # the lowest offending row is reported
        idx[b + 1] = idx[b]
        val[ptr[60]] = 0.0
    elif name == "same_rule_twice":                # one rule broken in two rows: the lower row
        idx[b + 1] = idx[b]
        idx[ptr[60] + 1] = idx[ptr[60]]
    elif name == "both_rules":                    # of two rules broken in one row, the lower-numbered one
        idx[b + 1] = idx[b]
        val[b + 3] = 0.0
    assert R.first_violation(ptr, idx, val, I) == (rule, row)
    rc, rn, st = _norms(gpu_device, ptr, idx, val, I)
    assert rc == -22 and st.host().tolist() == [rule, row]
    assert rn.untouched(), "rnorm must be untouched after a refusal"
    msg = _lib.lib().rk_last_error().decode()
    assert f"rule {rule}" in msg and f"row {row}" in msg


@pytest.mark.parametrize("n,rule", [(133144, 0), (133145, 3), (133153, 3)])
def test_norms_limit(gpu_device, n, rule):
    """n items rated 127: n_u = 16129 n reaches 2^31 at n = 133145 (the sum must be formed in 64 bits to see it)."""
    ptr = np.array([0, 3, 3 + n, 5 + n], dtype=np.int32)
    idx = np.r_[[0, 1, 2], np.arange(n), [4, 9]].astype(np.int32)
    val = np.r_[[1, 2, 3], np.full(n, 127), [5, 5]].astype(np.float32)
    rc, rn, st = _norms(gpu_device, ptr, idx, val, 133153)
    if rule:
        assert rc == -22 and st.host().tolist() == [3, 1] and rn.untouched()
    else:
        n_u = np.array([14, 16129 * n, 50], dtype=np.int64)
        assert rc == 0 and st.host().tolist() == [0, -1]
        assert np.array_equal(rn.host(), (1.0 / np.sqrt(n_u.astype(np.float64))).astype(np.float32))


def test_norms_bad_arguments(gpu_device):
    rows, vals, I = _norm_rows("implicit")
    ptr, idx, val = _csr(rows, vals)
    rn, st = Out(70, torch.float32, gpu_device), Out(2, torch.int32, gpu_device)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, gpu_device) for a in (ptr, idx, val)]
    assert L.rk_knn_norms(0, I, P(d[0]), P(d[1]), P(d[2]), P(rn.full), P(st.full), S(gpu_device)) == -22
    assert L.rk_knn_norms(70, I, P(d[0]), P(d[1]), P(d[2]), None, P(st.full), S(gpu_device)) == -22
    assert L.rk_knn_norms(70, I, P(d[0]), P(d[1]), P(d[2]), P(rn.full), None, S(gpu_device)) == -22
    torch.cuda.synchronize()
    assert rn.untouched() and st.untouched()


# ------------------------------------------------------------------------------------------------------------ rk_knn_degsim
def _degsim(dev, csr, n_items, k, band, order=None, want_topw=True):
    ptr, idx, val = csr
    U = len(ptr) - 1
    colptr, crow, cval = _transpose(ptr, idx, val, n_items)
    rnorm = R.rnorm(R.dense(ptr, idx, val, n_items))
    topw, deg = Out(U * k, torch.float32, dev), Out(U, torch.float32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, dev) for a in (ptr, idx, val, colptr, crow, cval, rnorm)]
    d_order = None if order is None else _dev(np.asarray(order, dtype=np.int32), dev)
    rc = L.rk_knn_degsim(U, n_items, *(P(t) for t in d), k, band, P(d_order), P(topw.full) if want_topw else None, P(deg.full), S(dev))
    torch.cuda.synchronize()
    return rc, topw, deg


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _check(dev, csr, n_items, k, band, **kw):
    want_topw, want_deg = R.degsim(*csr, n_items, k)
    rc, topw, deg = _degsim(dev, csr, n_items, k, band, **kw)
    assert rc == 0, _lib.lib().rk_last_error()
    got_deg = deg.host()
    assert _same_bits(got_deg, want_deg), np.nonzero(got_deg.view(np.uint32) != want_deg.view(np.uint32))[0][:10]
    if kw.get("want_topw", True):
        got = topw.host().reshape(len(want_deg), k)
        assert _same_bits(got, want_topw), np.argwhere(got.view(np.uint32) != want_topw.view(np.uint32))[:10]
    else:
        assert topw.untouched()
    return want_topw, want_deg


def _random_csr(U, I, mean_len, explicit, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.choice(I, size=int(min(I, n)), replace=False) for n in rng.integers(0, 2 * mean_len + 1, size=U)]
    vals = [rng.integers(1, 6, size=len(r)) for r in rows] if explicit else None
    return _csr(rows, vals)


@pytest.mark.parametrize("band", [64, 128])
@pytest.mark.parametrize("U", [1, 2, 63, 64, 65, 128, 129, 193])
def test_degsim_user_counts(gpu_device, U, band):
    """Every user is first, inside or last in some band; k = 25 exceeds U - 1 at U = 1, 2."""
    _check(gpu_device, _random_csr(U, 90, 12, U % 2 == 0, U), 90, 25, band)


@functools.lru_cache(maxsize=None)
def _far_neighbours():
    """193 users in bands of 64.  User 0 shares its 30 private items only with users 180..192 (the LAST band: the running list
    filled from the first bands is displaced), user 100 only with users 1..13 (the FIRST band: the list it filled there is kept
    through the later bands); everybody also has a few background items, so every band holds weaker candidates."""
    rng = np.random.default_rng(42)
    rows = [list(rng.choice(60, size=6, replace=False)) for _ in range(193)]
    for v in range(180, 193):
        rows[v] += list(100 + rng.choice(30, size=25, replace=False))
    rows[0] += list(range(100, 130))
    for v in range(1, 14):
        rows[v] += list(200 + rng.choice(30, size=25, replace=False))
    rows[100] += list(range(200, 230))
    return _csr(rows), 230


@pytest.mark.parametrize("band", [64, 128])
def test_degsim_neighbours_in_the_last_and_first_band(gpu_device, band):
    csr, I = _far_neighbours()
    topw, _ = _check(gpu_device, csr, I, 10, band)
    A = R.dense(*csr, I)
    W = (A @ A.T) / np.sqrt(np.outer((A * A).sum(1), (A * A).sum(1)))
    assert set(np.argsort(-W[0])[1:11]) <= set(range(180, 193)) and set(np.argsort(-W[100])[1:11]) <= set(range(1, 14))
    assert topw[0, 9] > 0.5 and topw[100, 9] > 0.5


@pytest.mark.parametrize("k", [1, 2, 25, 64, 128])
def test_degsim_k(gpu_device, k):
    """U = 65: k = 64 = U - 1 and k = 128 > U - 1 (k_eff = 64, the rest of topw is zero padding)."""
    want, _ = _check(gpu_device, _random_csr(65, 40, 10, True, 7), 40, k, 64)
    if k == 128:
        assert not want[:, 64:].any()


def test_degsim_row_and_column_lengths(gpu_device):
    """Rows of 0, 1, 63, 64, 65 and 600 items; columns held by 1, 63, 64, 65 and 257 users; one item that everybody has."""
    rng = np.random.default_rng(3)
    U, I = 300, 700
    rows = [set(rng.choice(np.arange(10, 600), size=int(n), replace=False).tolist()) for n in rng.integers(5, 30, size=U)]
    for u, n in zip((0, 1, 2, 3, 4, 5, 299), (0, 1, 63, 64, 65, 600, 0)):
        rows[u] = set(rng.choice(np.arange(10, 700), size=n, replace=False).tolist())
    for r in rows:
        r -= {0, 1, 2, 3, 4}
    for item, n in zip((0, 1, 2, 3, 4), (1, 63, 64, 65, 257)):
        for u in rng.choice(np.arange(6, 299), size=n, replace=False):
            rows[u].add(item)
    keep_empty = (0, 299)
    for u in range(U):
        if u not in keep_empty:
            rows[u].add(9)                          # the item every (non-empty) user has
    rows = [sorted(r) for r in rows]
    csr = _csr(rows, [rng.integers(1, 6, size=len(r)) for r in rows])
    colptr, _, _ = _transpose(*csr, I)
    assert [len(r) for r in (rows[0], rows[299])] == [0, 0] and {len(rows[u]) for u in (1, 2, 3, 4, 5)} >= {2, 64, 65, 66}
    assert np.diff(colptr)[:5].tolist() == [1, 63, 64, 65, 257] and np.diff(colptr)[9] == U - 2
    for band in (64, 128):
        _, deg = _check(gpu_device, csr, I, 25, band)
        assert deg[0] == 0 and deg[299] == 0


def test_degsim_exact_row_lengths(gpu_device):
    """Rows of exactly 0, 1, 63, 64, 65 and 600 items (nothing added to them), over 650 items."""
    rng = np.random.default_rng(8)
    rows = [rng.choice(650, size=n, replace=False) for n in (0, 1, 63, 64, 65, 600)] + [rng.choice(650, size=20, replace=False) for _ in range(64)]
    _check(gpu_device, _csr(rows), 650, 25, 64)


@pytest.mark.parametrize("band", [64, 128])
def test_degsim_identical_profiles(gpu_device, band):
    """Every w is the same number: the select's threshold has U - 2 copies in every band."""
    csr = _csr([[3, 5, 8, 13, 21]] * 150, [[5, 4, 3, 2, 1]] * 150)
    topw, deg = _check(gpu_device, csr, 30, 25, band)
    assert len(np.unique(topw)) == 1 and len(np.unique(deg)) == 1


def test_degsim_large_dots(gpu_device):
    ptr = np.array([0, 1100, 2200, 2201], dtype=np.int32)
    idx = np.r_[np.arange(1100), np.arange(1100), [5]].astype(np.int32)
    val = np.r_[np.full(2200, 127.0), [1.0]].astype(np.float32)
    topw, _ = _check(gpu_device, (ptr, idx, val), 1100, 2, 64)
    assert topw[0].tolist() == [np.float32(0.99999994), np.float32(0.030151134)]
    p, i, v, I = R.large_dot_odd()                   # an odd dot above 2^24: the int -> float conversion rounds
    _check(gpu_device, (p.astype(np.int32), i, v), I, 1, 64)


def test_degsim_automatic_band(gpu_device):
    _check(gpu_device, _random_csr(1300, 400, 20, True, 21), 400, 25, 0)


def test_degsim_maximal_band(gpu_device):
    """The largest band (all of a CU's LDS) on a small problem: one band, most of it unused."""
    _check(gpu_device, _random_csr(129, 90, 12, False, 5), 90, 25, _lib.RK_KNN_MAX_BAND)


@pytest.mark.parametrize("order", ["null", "identity", "reversed", "random"])
def test_degsim_order(gpu_device, order):
    csr, I = _far_neighbours()
    perm = {"null": None, "identity": np.arange(193), "reversed": np.arange(193)[::-1],
            "random": np.random.default_rng(1).permutation(193)}[order]
    _check(gpu_device, csr, I, 25, 64, order=perm)


def test_degsim_without_topw(gpu_device):
    csr, I = _far_neighbours()
    _check(gpu_device, csr, I, 25, 128, want_topw=False)


@pytest.mark.parametrize("k,band", [(0, 64), (129, 64), (25, 96), (25, 32), (25, _lib.RK_KNN_MAX_BAND + 64), (25, -64)])
def test_degsim_refusals_write_nothing(gpu_device, k, band):
    rc, topw, deg = _degsim(gpu_device, _random_csr(65, 40, 10, False, 2), 40, k, band)
    assert rc == -22 and topw.untouched() and deg.untouched()


# ------------------------------------------------------------------------------------------------------------ rk_knn_select
def _select(dev, scores, m, largest):
    out = Out(m, torch.int32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = _dev(np.asarray(scores, dtype=np.float32), dev)
    rc = L.rk_knn_select(len(scores), P(d), m, largest, P(out.full), S(dev))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("largest", [0, 1])
def test_select(gpu_device, largest):
    rng = np.random.default_rng(9)
    how = "high" if largest else "low"
    cases = {"random": rng.random(1000).astype(np.float32), "ties": rng.integers(0, 7, size=777).astype(np.float32) / 8,
             "equal": np.full(300, 0.25, dtype=np.float32),
             "zeros": np.array([0.5, -0.0, 0.0, -0.0, 0.25, 0.0, -1.0, 2.0], dtype=np.float32)}
    for name, s in cases.items():
        for m in (0, 1, len(s) // 2, len(s)):
            rc, out = _select(gpu_device, s, m, largest)
            assert rc == 0 and out.host().tolist() == R.select(s, m, how), (name, m)
    rc, out = _select(gpu_device, cases["zeros"], 8, largest)
    zeros = [i for i in out.host().tolist() if i in (1, 2, 3, 5)]
    assert zeros == [1, 2, 3, 5], "-0.0 and 0.0 are equal: the lower id first"


def test_select_refusals(gpu_device):
    s = np.array([0.1, np.nan, 0.3], dtype=np.float32)
    rc, _ = _select(gpu_device, s, 2, 0)
    assert rc == -22 and "rk_knn_select" in _lib.lib().rk_last_error().decode() and "non-finite" in _lib.lib().rk_last_error().decode()
    s[1] = np.inf
    assert _select(gpu_device, s, 2, 1)[0] == -22
    s[1] = 0.2
    rc, out = _select(gpu_device, s, 4, 0)
    assert rc == -22 and out.untouched()
    out = Out(3, torch.int32, gpu_device)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = _dev(s, gpu_device)
    assert L.rk_knn_select(3, P(d), -1, 0, P(out.full), S(gpu_device)) == -22 and out.untouched()
