"""GPU tests of the EASE kernels one entry point at a time (csrc/ease.hip) against the numpy restatement
(tests/_ease_restate.py).  The Gram matrix, the weights and the scores are compared bit for bit; the inverse is held to the
per-input budget e_P of the restatement (inside the hard bound I * 2^-24 * kappa * max|P*|, and within 4 x the fp32 walk's error
plus 2^-23 max|P*|).  Every buffer a kernel writes lies between two 64-element margins of NaN (ints: a sentinel) that must stay as
they were.  The refused matrices (a zero, a negative and a NaN pivot) are refusals the call returns from, not faults."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _ease_restate as R
from tests.test_knn_kernels_gpu import _dev, _transpose

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL = 64, -777
CAP = _lib.RK_EASE_MAX_ITEMS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Guarded:
    """n elements on the device between two margins of NaN (floats) or SENTINEL (ints); `init` fills the middle."""

    def __init__(self, n, dtype, dev, init=None):
        self.n, self.fp = int(n), dtype.is_floating_point
        self.full = torch.full((self.n + 2 * MARGIN,), float("nan") if self.fp else SENTINEL, dtype=dtype, device=dev)
        self.mid = self.full[MARGIN: MARGIN + self.n]
        if init is not None:
            self.mid.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dev))

    def _same(self, a):
        return bool(np.isnan(a).all() if self.fp else (a == SENTINEL).all())

    def margins_intact(self):
        full = self.full.cpu().numpy()
        return self._same(full[:MARGIN]) and self._same(full[MARGIN + self.n:])

    def host(self):
        assert self.margins_intact(), "the kernel wrote outside its buffer"
        return self.mid.cpu().numpy()

    def untouched(self):
        return self._same(self.full.cpu().numpy())


def _P(g):
    return _lib.ptr(g.mid if isinstance(g, Guarded) else g)


# --------------------------------------------------------------------------------------------------------------- rk_ease_gram
def _gram(dev, X, lam, n_items=None, drop=None):
    U, n = X.shape
    n_items = n if n_items is None else n_items
    ptr, idx, val = R.csr_of(X)
    colptr, crow, cval = _transpose(ptr, idx, val, n)
    A, st = Guarded(n * n, torch.float32, dev), Guarded(2, torch.int32, dev)
    d = [_dev(a, dev) for a in (ptr, idx, val, colptr, crow, cval)]     # held until the call has returned
    args = [_lib.ptr(t) for t in d] + [float(lam), _P(A), _P(st)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ease_gram(U, n_items, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, A, st


@pytest.mark.parametrize("block,n", R.SIZES)
def test_gram_equals_the_integer_product(gpu_device, block, n):
    for U, lam, explicit in R.CASES:
        c = R.case(block, n, U, lam, explicit)
        rc, A, st = _gram(gpu_device, c["X"], lam)
        assert rc == 0, _lib.lib().rk_last_error()
        got = A.host().reshape(n, n)
        assert np.array_equal(_bits(got), _bits(c["A"])), (U, lam, np.argwhere(_bits(got) != _bits(c["A"]))[:5])
        assert st.host().tolist() == [0, -1]


def test_gram_over_two_bands(gpu_device):
    """8192 + 65 items: the accumulators hold 8192 columns, so every row of A takes the band loop twice.  User 0 has some 300
    entries over both bands (more than 128: its band segment is binary-searched), the other 39 have 6 to 102, fewer than 128
    (strided whole and filtered); items 8191 and 8192, either side of the band edge, are rated by users 0 to 3.  The expected
    matrix is built from the integer products of each user's entries; every bit of A is compared."""
    n, U, lam = 8192 + 65, 40, 2.5
    rng = np.random.default_rng(8257)
    X = np.zeros((U, n), dtype=np.int64)
    for u in range(U):
        cnt = 300 if u == 0 else 6 + (u * 37) % 95
        X[u, rng.choice(n, size=cnt, replace=False)] = rng.integers(1, 6, size=cnt)
    X[:4, 8191:8193] = [[5, 1], [2, 3], [1, 1], [4, 2]]
    lens = (X != 0).sum(axis=1)
    assert lens[0] > 128 and lens[1:].max() < 128 and (X[0, :8192] != 0).sum() > 0 < (X[0, 8192:] != 0).sum()
    D = np.zeros(n * n, dtype=np.int32)
    for u in range(U):
        c = np.nonzero(X[u])[0]
        np.add.at(D, (c[:, None] * n + c[None, :]).reshape(-1), np.outer(X[u, c], X[u, c]).reshape(-1))
    assert D.max() < 2 ** 24 and D[8191 * n + 8192] == 5 + 6 + 1 + 8
    want = D.astype(np.float32)
    del D
    want[:: n + 1] = (want[:: n + 1] + np.float32(lam)).astype(np.float32)
    rc, A, st = _gram(gpu_device, X, lam)
    assert rc == 0, _lib.lib().rk_last_error()
    got = A.host()
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    assert st.host().tolist() == [0, -1]


def _heavy_column(extra):
    """1044 (+ extra) users x 3 items: item 1 is rated 127 by 1040 users, then 55, 5, 2, 1: d_11 = 2^24 - 1; each extra user adds 1."""
    col = np.r_[np.full(1040, 127), [55, 5, 2, 1], np.ones(extra, dtype=np.int64)].astype(np.int64)
    X = np.zeros((len(col), 3), dtype=np.int64)
    X[:, 1] = col
    X[::3, 0] = 4
    X[5::7, 2] = 1
    return X


def test_gram_largest_diagonal_and_its_refusal(gpu_device):
    X = _heavy_column(0)
    D = R.gram(X)
    assert D[1, 1] == 2 ** 24 - 1 and D[0, 1] > 0
    rc, A, st = _gram(gpu_device, X, 0.5)
    assert rc == 0, _lib.lib().rk_last_error()
    assert np.array_equal(_bits(A.host().reshape(3, 3)), _bits(R.matrix(D, 0.5))) and st.host().tolist() == [0, -1]
    X = _heavy_column(1)
    assert R.gram(X)[1, 1] == 2 ** 24
    rc, A, st = _gram(gpu_device, X, 0.5)
    assert rc == -22 and A.untouched(), "A is untouched on the refusal"
    assert st.host().tolist() == [_lib.RK_EASE_BAD_GRAM, 1] and "item 1" in _lib.lib().rk_last_error().decode()
    X[:, 2] = X[:, 1]                              # a second item over the limit: the lower one is reported
    rc, A, st = _gram(gpu_device, X, 0.5)
    assert rc == -22 and A.untouched() and st.host().tolist() == [_lib.RK_EASE_BAD_GRAM, 1]


@pytest.mark.parametrize("lam,n_items,drop", [(float("nan"), None, None), (0.0, None, None), (-1.0, None, None), (float("inf"), None, None),
                                              (1.0, 0, None), (1.0, -3, None), (1.0, CAP + 1, None), (1.0, None, 0), (1.0, None, 5),
                                              (1.0, None, 7), (1.0, None, 8)])
def test_gram_refusals_write_nothing(gpu_device, lam, n_items, drop):
    rc, A, st = _gram(gpu_device, R.ratings(20, 9, 3), lam, n_items=n_items, drop=drop)
    assert rc == -22 and A.untouched() and st.untouched()
    assert "rk_ease_gram" in _lib.lib().rk_last_error().decode()


# ------------------------------------------------------------------------------------------------------------- rk_ease_invert
def _invert(dev, A, block, n=None, work_floats=None, drop=None):
    A = np.asarray(A, dtype=np.float32)
    n = len(A) if n is None else n
    b = R.resolved_block(len(A), block) if block in (0,) + R.BLOCKS else 128     # an unsupported block gets the largest workspace
    a = Guarded(A.size, torch.float32, dev, init=A)
    work, st = Guarded(len(A) * b, torch.float32, dev), Guarded(2, torch.int32, dev)
    args = [_P(a), _P(work), work.n if work_floats is None else work_floats, block, _P(st)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ease_invert(n, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, a, work, st


@pytest.mark.parametrize("block,n", R.SIZES)
def test_invert_holds_the_budget_and_repeats(gpu_device, block, n):
    worst = worst_rel = worst_hard = 0.0
    for U, lam, explicit in R.CASES:
        c = R.case(block, n, U, lam, explicit)
        rc, a, work, st = _invert(gpu_device, c["A"], block)
        assert rc == 0, _lib.lib().rk_last_error()
        P = a.host().reshape(n, n)
        assert work.margins_intact() and st.host().tolist() == [0, -1]
        err = float(np.max(np.abs(P.astype(np.float64) - c["P_star"])))
        print(f"block {block} I {n} U {U} lambda {lam}{' 1..5' if explicit else ''}: device error {err:.3e} = {err / c['max_P']:.1e} max|P*| = "
              f"{err / c['e_hard']:.4f} of the hard bound, walk {c['walk_err']:.3e}, budget {c['e_P']:.3e}")
        assert np.all(np.isfinite(P)) and err <= c["e_hard"], (U, lam, err, c["e_hard"])
        assert err <= c["e_P"], (U, lam, err, c["e_P"])
        rc, again, _, _ = _invert(gpu_device, c["A"], block)
        assert rc == 0 and np.array_equal(_bits(again.host()), _bits(P.reshape(-1))), "two runs give the same bits"
        worst, worst_rel, worst_hard = max(worst, err / c["e_P"]), max(worst_rel, err / c["max_P"]), max(worst_hard, err / c["e_hard"])
    print(f"block {block} I {n}: device error <= {worst_rel:.1e} max|P*|, <= {worst_hard:.4f} of the hard bound, <= {worst:.3f} of the budget")


@functools.lru_cache(maxsize=None)
def _spd(n):
    A = R.matrix(R.gram(R.ratings(200, n, 77)), 10.0).copy()
    return A


@pytest.mark.parametrize("block", [32, 64, 0])
@pytest.mark.parametrize("kind,at", [("zero", 0), ("zero", 70), ("zero", 149), ("negative", 33), ("negative", 149), ("nan", 64),
                                     ("nan", 130), ("nan_off_diagonal", (20, 101)), ("inf", 5), ("two_zeros", (33, 120))])
def test_invert_refuses_a_bad_pivot(gpu_device, kind, at, block):
    """150 items: the bad pivot in the first block, in a later one or in the last, partial one.  Row and column z are cleared and
    the diagonal set, so pivot z is exactly that value; a NaN at (i, j) first reaches a pivot at max(i, j); of two bad pivots the
    lower is reported."""
    A = _spd(150).copy()
    if kind == "nan_off_diagonal":
        A[at] = np.nan
        z = max(at)
    elif kind == "two_zeros":
        z = min(at)
        A[list(at), :] = 0
        A[:, list(at)] = 0
    else:
        z = at
        A[z, :] = 0
        A[:, z] = 0
        A[z, z] = {"zero": 0.0, "negative": -1.0, "nan": np.nan, "inf": np.inf}[kind]
    P_walk, bad = R.invert_walk(A, block)
    assert P_walk is None and bad == z
    rc, a, work, st = _invert(gpu_device, A, block)
    assert rc == -22 and st.host().tolist() == [_lib.RK_EASE_NOT_SPD, z], (rc, st.host())
    assert a.margins_intact() and work.margins_intact() and f"pivot {z} " in _lib.lib().rk_last_error().decode()


@pytest.mark.parametrize("n,block,work_floats,drop", [(0, 0, None, None), (-1, 0, None, None), (CAP + 1, 0, None, None), (70, 16, None, None),
                                                      (70, 48, None, None), (70, 128, None, None), (70, -32, None, None), (70, 1, None, None),
                                                      (70, 64, 70 * 64 - 1, None), (70, 0, 70 * 64 - 1, None), (70, 32, 70 * 32 - 1, None),
                                                      (70, 32, -1, None), (70, 0, None, 0), (70, 0, None, 1), (70, 0, None, 4)])
def test_invert_refusals_write_nothing(gpu_device, n, block, work_floats, drop):
    A = _spd(70)
    rc, a, work, st = _invert(gpu_device, A, block, n=n, work_floats=work_floats, drop=drop)
    assert rc == -22 and work.untouched() and st.untouched()
    assert a.margins_intact() and np.array_equal(_bits(a.host()), _bits(A.reshape(-1)))
    assert "rk_ease_invert" in _lib.lib().rk_last_error().decode()


# ------------------------------------------------------------------------------------------------------------ rk_ease_weights
def _weights(dev, P, in_place, n=None, drop=None):
    P = np.asarray(P, dtype=np.float32)
    n = len(P) if n is None else n
    p = Guarded(P.size, torch.float32, dev, init=P)
    b = p if in_place else Guarded(P.size, torch.float32, dev)
    args = [_P(p), _P(b)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ease_weights(n, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, p, b


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 300])
def test_weights_equal_the_restatement(gpu_device, n, in_place):
    """An asymmetric P (so that a transposed divisor shows), with zeros, negatives and a wide range of magnitudes."""
    rng = np.random.default_rng(n)
    P = (rng.standard_normal((n, n)) * 10.0 ** rng.integers(-6, 3, size=(n, n))).astype(np.float32)
    P[rng.random((n, n)) < 0.05] = 0
    P[np.arange(n), np.arange(n)] = (rng.random(n) + 0.01).astype(np.float32)
    want = R.weights(P)
    if n > 1:
        assert not np.array_equal(want, R.weights(P.T).T)
    rc, p, b = _weights(gpu_device, P, in_place)
    assert rc == 0, _lib.lib().rk_last_error()
    got = b.host().reshape(n, n)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    assert np.all(_bits(got[np.arange(n), np.arange(n)]) == 0)
    if not in_place:
        assert np.array_equal(_bits(p.host()), _bits(P.reshape(-1))), "P is only read"


def test_weights_from_an_inverse(gpu_device):
    c = R.case(0, 200, 300, 500.0)
    rc, _, b = _weights(gpu_device, c["P_walk"], True)
    assert rc == 0 and np.array_equal(_bits(b.host().reshape(200, 200)), _bits(R.weights(c["P_walk"])))


@pytest.mark.parametrize("n,drop", [(0, None), (-5, None), (CAP + 1, None), (9, 0), (9, 1)])
def test_weights_refusals_write_nothing(gpu_device, n, drop):
    P = _spd(9)
    rc, p, b = _weights(gpu_device, P, False, n=n, drop=drop)
    assert rc == -22 and b.untouched() and np.array_equal(_bits(p.host()), _bits(P.reshape(-1)))
    assert "rk_ease_weights" in _lib.lib().rk_last_error().decode()


# ------------------------------------------------------------------------------- rk_ease_scores / rk_ease_pair_scores
@functools.lru_cache(maxsize=None)
def _score_input(n):
    """40 users over n items with ratings 1..5 and a few 127: user 0 has no entries, user 1 has rated everything."""
    X = R.ratings(40, n, 500 + n, explicit=True).copy()
    X[np.nonzero(X)[0][::11], np.nonzero(X)[1][::11]] = 127
    X[0] = 0
    X[1] = 1 + np.arange(n) % 5
    return X


def _device_B(dev, X, lam, block):
    """B by the device's own fit (gram, invert, weights in place), as a device tensor and on the host."""
    n = X.shape[1]
    rc, A, _ = _gram(dev, X, lam)
    assert rc == 0, _lib.lib().rk_last_error()
    b = R.resolved_block(n, block)
    work, st = torch.empty(n * b, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    L, s = _lib.lib(), _lib.stream_ptr(dev)
    _lib.check(L.rk_ease_invert(n, _P(A), _lib.ptr(work), work.numel(), block, _lib.ptr(st), s), "rk_ease_invert")
    _lib.check(L.rk_ease_weights(n, _P(A), _P(A), s), "rk_ease_weights")
    torch.cuda.synchronize()
    return A, A.host().reshape(n, n).copy()


def _scores(dev, X, B, users, n_items=None, nb=None, drop=None):
    n = X.shape[1]
    ptr, idx, val = R.csr_of(X)
    out = Guarded(len(users) * n, torch.float32, dev)
    d = [_dev(a, dev) for a in (ptr, idx, val, np.asarray(users, dtype=np.int32))]
    args = [_P(B), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), len(users) if nb is None else nb, _lib.ptr(d[3]), _P(out)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ease_scores(n if n_items is None else n_items, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out


def _pairs(dev, X, B, users, items, n_items=None, drop=None):
    U, n = X.shape
    ptr, idx, val = R.csr_of(X)
    out = Guarded(len(users), torch.float32, dev)
    d = [_dev(a, dev) for a in (ptr, idx, val, np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64))]
    args = [_P(B)] + [_lib.ptr(t) for t in d] + [len(users), _P(out)]
    if drop is not None:
        args[drop] = None
    rc = _lib.lib().rk_ease_pair_scores(n if n_items is None else n_items, U, *args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("block,n", R.SIZES)
def test_scores_and_pairs_equal_the_chain_over_the_device_weights(gpu_device, block, n):
    X = _score_input(n)
    B_dev, B = _device_B(gpu_device, X, 10.0, block)
    assert np.all(np.isfinite(B)) and np.all(_bits(np.diag(B)) == 0)
    users = np.r_[np.arange(40), [0, 1, 1, 7, 39, 7]]                   # every user, then the empty one, the full one and repeats
    want = R.scores(X, B, users)
    rc, out = _scores(gpu_device, X, B_dev, users)
    assert rc == 0, _lib.lib().rk_last_error()
    got = out.host().reshape(len(users), n)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
    assert np.all(_bits(got[0]) == 0) and np.array_equal(_bits(got[1]), _bits(got[41])) and (n < 2 or got[1].any())
    # 500 pairs, ids out of range among them: the same bits as the matrix entries
    rng = np.random.default_rng(n)
    pu, pi = rng.integers(0, 40, size=500), rng.integers(0, n, size=500)
    bad = [(-1, 0), (40, 0), (3, -1), (3, n), (2 ** 40, 0), (3, 2 ** 40), (-2 ** 40, -2 ** 40), (40, n)]
    for k, (u, i) in enumerate(bad):
        pu[100 + k], pi[100 + k] = u, i
    pu[:3] = [0, 1, 1]
    rc, pout = _pairs(gpu_device, X, B_dev, pu, pi)
    assert rc == 0, _lib.lib().rk_last_error()
    pgot = pout.host()
    assert np.array_equal(_bits(pgot), _bits(R.pair_scores(X, B, pu, pi)))
    ok = np.ones(500, dtype=bool)
    ok[100:108] = False
    assert np.array_equal(_bits(pgot[ok]), _bits(got[pu[ok], pi[ok]])) and np.all(_bits(pgot[100:108]) == 0)


def test_scores_rows_longer_than_one_staging_chunk(gpu_device):
    """600 items and users with 0, 255, 256, 257, 513 and 600 entries: the kernel stages 256 entries at a time."""
    n = 600
    rng = np.random.default_rng(4)
    X = np.zeros((6, n), dtype=np.int64)
    for u, cnt in enumerate((0, 255, 256, 257, 513, 600)):
        X[u, np.sort(rng.choice(n, size=cnt, replace=False))] = rng.integers(1, 6, size=cnt)
    B = (rng.standard_normal((n, n)) * 0.1).astype(np.float32)
    B_dev = torch.from_numpy(B).to(gpu_device).reshape(-1)
    users = [5, 0, 3, 2, 1, 4, 3]
    rc, out = _scores(gpu_device, X, B_dev, users)
    assert rc == 0 and np.array_equal(_bits(out.host().reshape(len(users), n)), _bits(R.scores(X, B, users)))
    pu, pi = rng.integers(0, 6, size=500), rng.integers(0, n, size=500)
    rc, pout = _pairs(gpu_device, X, B_dev, pu, pi)
    assert rc == 0 and np.array_equal(_bits(pout.host()), _bits(R.pair_scores(X, B, pu, pi)))


def test_scores_and_pairs_with_nothing_to_do(gpu_device):
    X = _score_input(9)
    B_dev = torch.zeros(81, device=gpu_device)
    rc, out = _scores(gpu_device, X, B_dev, [])
    assert rc == 0 and out.untouched()
    rc, pout = _pairs(gpu_device, X, B_dev, [], [])
    assert rc == 0 and pout.untouched()


@pytest.mark.parametrize("n_items,nb,drop", [(0, None, None), (-1, None, None), (CAP + 1, None, None), (None, -1, None), (None, None, 0),
                                             (None, None, 1), (None, None, 5), (None, None, 6)])
def test_scores_refusals_write_nothing(gpu_device, n_items, nb, drop):
    X = _score_input(9)
    rc, out = _scores(gpu_device, X, torch.zeros(81, device=gpu_device), [1, 2, 3], n_items=n_items, nb=nb, drop=drop)
    assert rc == -22 and out.untouched() and "rk_ease_scores" in _lib.lib().rk_last_error().decode()


@pytest.mark.parametrize("n_items,drop", [(0, None), (CAP + 1, None), (None, 0), (None, 1), (None, 4), (None, 5), (None, 7)])
def test_pairs_refusals_write_nothing(gpu_device, n_items, drop):
    X = _score_input(9)
    rc, out = _pairs(gpu_device, X, torch.zeros(81, device=gpu_device), [1, 2, 3], [0, 1, 2], n_items=n_items, drop=drop)
    assert rc == -22 and out.untouched() and "rk_ease_pair_scores" in _lib.lib().rk_last_error().decode()
