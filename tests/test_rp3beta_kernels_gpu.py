"""GPU tests of the RP3beta kernels one entry point at a time (csrc/rp3beta.hip) against the numpy restatement of the definition
(tests/_rp3_restate.py).  Every stage is fed from device inputs of its own: the neighbour entry from the P, fa and fb the device
wrote (read back and restated from) and from hand-made P tables, the scoring entries from the tables the device fitted.  r, ids
and the bit patterns of weights and scores are compared exactly; P away from exponents 0 and 1 within one unit and the factors
within the stated allowance of the double pow.  Every output buffer is pre-filled with NaN (ints: a sentinel) and carries a
64-element margin that must stay as it was."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _rp3_restate as R
from tests.test_itemknn_kernels_gpu import _bits, _dense_csr, _random_csr
from tests.test_knn_kernels_gpu import Out, _csr, _dev, _transpose

pytestmark = pytest.mark.gpu
# double pow: the OpenCL C specification asks 16 ulp of it, which is what the device math library is built to meet (no
# accuracy table ships with the toolkit); numpy's own pow gets one more
POW_ULP = 17.0


def _call(fn, dev, *args):
    rc = fn(*args, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc


def _err():
    return _lib.lib().rk_last_error().decode()


# ------------------------------------------------------------------------------------------------------------- rk_rp3_steps
def _steps(dev, csr, alpha, drop=None, n_users=None):
    ptr, idx, val = csr
    U = len(ptr) - 1
    P, r = Out(len(idx), torch.int64, dev), Out(U, torch.int64, dev)
    d = [_dev(a, dev) for a in (ptr.astype(np.int32), val)]            # held until the call has returned
    args = [_lib.ptr(d[0]), _lib.ptr(d[1]), float(alpha), _lib.ptr(P.full), _lib.ptr(r.full)]
    if drop is not None:
        args[drop] = None
    rc = _call(_lib.lib().rk_rp3_steps, dev, U if n_users is None else n_users, *args)
    return rc, P, r


@functools.lru_cache(maxsize=None)
def _step_rows():
    """70 users over 300 items: empty rows, a row of one, rows of 63, 64, 65 and 200 entries; ratings 1..5 and some 127."""
    rng = np.random.default_rng(41)
    lens = rng.integers(1, 90, size=70)
    lens[[0, 69]], lens[7], lens[[11, 12, 13]], lens[9] = 0, 1, (63, 64, 65), 200
    rows = [np.sort(rng.choice(300, size=int(n), replace=False)) for n in lens]
    vals = [np.where(rng.random(len(r)) < 0.1, 127, rng.integers(1, 6, size=len(r))) for r in rows]
    return _csr(rows, vals)


@pytest.mark.parametrize("alpha", [0, 1, 0.8, 2, 0.3, 4])
def test_steps(gpu_device, alpha):
    """r exactly; P exactly at alpha 0 and 1 (no pow); elsewhere |dP| <= 1: the two pows differ by at most 17 ulp of a p <= 1,
    which moves 2^40 p by 2^40 * 17 * 2^-53 = 2e-3, so the rounded integers differ only next to a half, and then by one."""
    csr = _step_rows()
    want_P, want_r = R.steps(*csr, alpha)
    rc, P, r = _steps(gpu_device, csr, alpha)
    assert rc == 0, _err()
    got_P, got_r = P.host(), r.host()
    assert np.array_equal(got_r, want_r) and want_r[0] == 0 and want_r.max() > 127
    diff = np.abs(got_P - want_P)
    print(f"alpha={alpha}: {int(np.sum(diff > 0))} of {len(diff)} P differ from numpy's, the largest by {int(diff.max())}")
    assert np.all(got_P >= 1) and np.all(got_P <= 2 ** 40)
    if alpha in (0, 1):
        assert np.array_equal(got_P, want_P)
    else:
        assert diff.max() <= 1


def test_steps_keep_a_vanishing_step_at_one(gpu_device):
    """(1 / 1398)^4 * 2^40 rounds to 0: P = 1 (the user of tests/test_rp3beta_host.py)."""
    csr = _csr([np.arange(12), [12]], [[1] + [127] * 11, [3]])
    rc, P, r = _steps(gpu_device, csr, 4)
    assert rc == 0 and r.host().tolist() == [1398, 3] and P.host()[0] == 1 and P.host()[12] == 2 ** 40 and np.all(P.host()[1:12] > 1)


@pytest.mark.parametrize("alpha,drop,n_users", [(-0.1, None, None), (4.5, None, None), (float("nan"), None, None),
                                                (float("inf"), None, None), (1, 0, None), (1, 1, None), (1, 3, None), (1, 4, None),
                                                (1, None, _lib.RK_RP3_MAX_USERS), (1, None, 0)])
def test_steps_refusals_write_nothing(gpu_device, alpha, drop, n_users):
    rc, P, r = _steps(gpu_device, _step_rows(), alpha, drop=drop, n_users=n_users)
    assert rc == -22 and P.untouched() and r.untouched() and "rk_rp3_steps" in _err()


# ----------------------------------------------------------------------------------------------------------- rk_rp3_factors
COUNTS = np.array([0, 1, 2, 3, 0, 7, 64, 1000, 65537, 2 ** 23 - 1, 5, 0] + list(range(1, 120)), dtype=np.int64)


def _factors(dev, counts, alpha, beta, drop=None):
    I = len(counts)
    fa, fb = Out(I, torch.float64, dev), Out(I, torch.float64, dev)
    colptr = _dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), dev)
    args = [_lib.ptr(colptr), float(alpha), float(beta), _lib.ptr(fa.full), _lib.ptr(fb.full)]
    if drop is not None:
        args[drop] = None
    return _call(_lib.lib().rk_rp3_factors, dev, I, *args), fa, fb


@pytest.mark.parametrize("alpha,beta", [(1, 0), (0, 1), (1, 0.6), (0.8, 0.4), (2, 0.3), (4, 4), (0.5, 3.7)])
def test_factors(gpu_device, alpha, beta):
    """Exponents 0 and 1 exactly (1 and the IEEE quotient); the others within POW_ULP units of numpy's float64 power; an item
    nobody rated gives +0.0."""
    counts = COUNTS
    assert counts.sum() < 2 ** 31
    want = R.factors(counts, alpha, beta)
    rc, fa, fb = _factors(gpu_device, counts, alpha, beta)
    assert rc == 0, _err()
    for name, e, got, ref in (("fa", alpha, fa.host(), want[0]), ("fb", beta, fb.host(), want[1])):
        assert np.all(got.view(np.uint64)[counts == 0] == 0) and np.all(got[counts > 0] > 0)
        if e in (0, 1):
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), name
        else:
            ulps = np.abs(got - ref) / np.spacing(np.where(ref > 0, ref, 1.0))
            print(f"{name} exponent {e}: worst difference from numpy {ulps.max():.2f} ulp (allowance {POW_ULP})")
            assert ulps.max() <= POW_ULP, name


@pytest.mark.parametrize("alpha,beta,drop", [(-1, 0, None), (5, 0, None), (float("nan"), 0, None), (1, -0.5, None), (1, 4.01, None),
                                             (1, float("inf"), None), (1, 1, 0), (1, 1, 3), (1, 1, 4)])
def test_factors_refusals_write_nothing(gpu_device, alpha, beta, drop):
    rc, fa, fb = _factors(gpu_device, COUNTS[:40], alpha, beta, drop=drop)
    assert rc == -22 and fa.untouched() and fb.untouched() and "rk_rp3_factors" in _err()


# --------------------------------------------------------------------------------------------------------- rk_rp3_neighbors
def _device_parts(dev, csr, n_items, alpha, beta):
    """(P, fa, fb) as the device computes them, read back."""
    rc, P, _ = _steps(dev, csr, alpha)
    assert rc == 0, _err()
    rc2, fa, fb = _factors(dev, np.bincount(csr[1], minlength=n_items), alpha, beta)
    assert rc2 == 0, _err()
    return P.host().copy(), fa.host().copy(), fb.host().copy()


def _neighbors(dev, csr, n_items, k, band, P, fa, fb, order=None, drop=None, n_users=None):
    ptr, idx, val = csr
    U = len(ptr) - 1
    colptr, crow, _ = _transpose(ptr, idx, val, n_items)
    ids, w = Out(max(k, 1) * n_items, torch.int32, dev), Out(max(k, 1) * n_items, torch.float32, dev)
    d = [_dev(a, dev) for a in (ptr.astype(np.int32), idx, np.asarray(P, dtype=np.int64), colptr, crow,
                                np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64))]
    d_order = None if order is None else _dev(np.asarray(order, dtype=np.int32), dev)
    args = [_lib.ptr(t) for t in d]
    if drop is not None:
        args[drop] = None
    rc = _call(_lib.lib().rk_rp3_neighbors, dev, U if n_users is None else n_users, n_items, *args, k, band, _lib.ptr(d_order),
               _lib.ptr(ids.full), _lib.ptr(w.full))
    return rc, ids, w


def _restated(csr, n_items, P, fa, fb):
    S = R.dots(csr[0], csr[1], P, n_items)
    return S, R.weights(S, fa, fb)


def _check(dev, csr, n_items, k, band, parts, want=None, **kw):
    P, fa, fb = parts
    want_id, want_w = R.neighbours_from(*_restated(csr, n_items, P, fa, fb), k) if want is None else want
    rc, ids, w = _neighbors(dev, csr, n_items, k, band, P, fa, fb, **kw)
    assert rc == 0, _err()
    got_id, got_w = ids.host().reshape(k, n_items), w.host().reshape(k, n_items)
    assert np.array_equal(got_id, want_id), np.argwhere(got_id != want_id)[:10]
    assert np.array_equal(_bits(got_w), _bits(want_w)), np.argwhere(_bits(got_w) != _bits(want_w))[:10]
    return want_id, want_w


@pytest.mark.parametrize("U", [1, 5, 70])
@pytest.mark.parametrize("I", [1, 2, 3, 63, 64, 65, 129, 200])
def test_neighbors_shapes(gpu_device, I, U):
    """From the device's own P, fa and fb.  Every item is first, inside or last in some band of 64; k >= I - 1 pads, I = 1 has no
    candidate at all; user 0's row is empty when there are several users and item I - 2 has no rater.  At alpha = 1 the device's
    parts are the definition's to the bit, so the tables are the definition's too."""
    csr = _random_csr(U, I, 0.5 if U < 70 else 0.15, (I + U) % 2 == 0, 100 * I + U, empty_rows=[0] if U > 1 else [],
                      empty_cols=[I - 2] if I > 2 else [])
    alpha, beta = ((1, 0.6), (0.8, 0.4), (2, 0.3))[(I + U) % 3]
    parts = _device_parts(gpu_device, csr, I, alpha, beta)
    SW = _restated(csr, I, *parts)
    for k in (1, 5, 50, 128):
        want_id, _ = _check(gpu_device, csr, I, k, 64, parts, want=R.neighbours_from(*SW, k))
        if k >= I:
            assert np.all(want_id[max(I - 1, 0):] == -1)
        if alpha == 1:
            pure = R.neighbours(*csr, I, k, alpha, beta)
            assert np.array_equal(pure[0], want_id), "alpha = 1: no pow anywhere, the device's P is the definition's"
    if I > 2:
        assert np.all(want_id[:, I - 2] == -1) and not np.any(want_id == I - 2)


@pytest.mark.parametrize("band", [64, 128, 0])
@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_neighbors_bands(gpu_device, kind, band):
    """I = 200: bands of 64 (last one 8 wide) and 128 (last one 72), and the automatic single band."""
    csr = list(_random_csr(90, 200, 0.12, kind != "implicit", 17, empty_rows=[3, 89], empty_cols=[0, 64, 199]))
    if kind == "value127":
        csr[2] = np.where(np.arange(len(csr[2])) % 3 == 0, np.float32(127), csr[2]).astype(np.float32)
    csr = tuple(csr)
    parts = _device_parts(gpu_device, csr, 200, 1, 0.6)
    SW = _restated(csr, 200, *parts)
    for k in (7, 50):
        _check(gpu_device, csr, 200, k, band, parts, want=R.neighbours_from(*SW, k))


@functools.lru_cache(maxsize=None)
def _tie_block():
    """70 users over 100 items: columns 10..49 are identical (the same steps, the same rater count), the rest random."""
    rng = np.random.default_rng(5)
    A = (rng.random((70, 100)) < 0.2) * rng.integers(1, 6, size=(70, 100))
    A[:, 10:50] = A[:, [10]]
    assert A[:, 10].any()
    csr = _dense_csr(A)
    P, _, fa, fb = R.fit_parts(*csr, 100, 1, 0.6)
    return csr, (P, fa, fb)


@pytest.mark.parametrize("band", [64, 0])
@pytest.mark.parametrize("k", [7, 25, 39, 64])
def test_neighbors_block_of_identical_columns(gpu_device, k, band):
    """Each of the 40 identical columns sees the 39 others at one weight: inside a run of equal weights the ids ascend, and a cut
    inside the run keeps the lowest."""
    csr, parts = _tie_block()
    want_id, want_w = _check(gpu_device, csr, 100, k, band, parts)
    col = want_id[:, 30]
    tied = [t for t in range(k) if 10 <= col[t] < 50]
    assert len(tied) >= min(k, 5) and len({_bits(want_w[t, 30]).item() for t in tied}) == 1
    assert col[tied].tolist() == [j for j in range(10, 50) if j != 30][: len(tied)]


@pytest.mark.parametrize("k", [1, 3, 5, 9, 10, 11])
def test_neighbors_tie_group_across_a_band_edge(gpu_device, k):
    """Columns 60..70 are identical and nothing else overlaps them: a cut inside the group keeps the lowest ids, whichever side
    of the edge between the bands [0, 64) and [64, 128) they lie on."""
    rng = np.random.default_rng(6)
    A = np.zeros((40, 130), dtype=np.int64)
    A[:20, :60] = rng.random((20, 60)) < 0.3
    A[:20, 71:] = rng.random((20, 59)) < 0.3
    A[20:, 60:71] = rng.integers(1, 6, size=(20, 1))
    csr = _dense_csr(A)
    P, _, fa, fb = R.fit_parts(*csr, 130, 1, 0.6)
    want_id, _ = _check(gpu_device, csr, 130, k, 64, (P, fa, fb))
    assert want_id[:, 60].tolist()[: min(k, 10)] == list(range(61, 71))[:k] and want_id[:, 70].tolist()[: min(k, 10)] == list(range(60, 70))[:k]


@pytest.mark.parametrize("band", [64, 128])
def test_neighbors_tie_group_in_a_later_band(gpu_device, band):
    """Columns 5..14 and 130..139 are all identical and rated by nobody else's pattern: the equal candidates of a later band must
    not displace the equal ones already listed."""
    rng = np.random.default_rng(7)
    A = np.zeros((50, 200), dtype=np.int64)
    col = rng.integers(1, 6, size=50) * (rng.random(50) < 0.5)
    A[:, 5:15] = col[:, None]
    A[:, 130:140] = col[:, None]
    csr = _dense_csr(A)
    P, _, fa, fb = R.fit_parts(*csr, 200, 1, 0.6)
    want_id, want_w = _check(gpu_device, csr, 200, 8, band, (P, fa, fb))
    assert want_id[:, 5].tolist() == list(range(6, 14)) and want_id[:, 135].tolist() == list(range(5, 13))
    assert len(np.unique(want_w[:, 5])) == 1


@functools.lru_cache(maxsize=None)
def _many_candidates(tied):
    """40 users over 700 items, dense: every item overlaps hundreds of others, so the pending area overflows and list and
    pending are merged several times per item.  tied: the columns are copies of 25 patterns (about 28 equal weights each)."""
    rng = np.random.default_rng(9)
    if tied:
        pat = (rng.random((40, 25)) < 0.35) * rng.integers(1, 4, size=(40, 25))
        A = pat[:, rng.integers(0, 25, size=700)]
    else:
        A = (rng.random((40, 700)) < 0.3) * rng.integers(1, 6, size=(40, 700))
    csr = _dense_csr(A)
    B = (A > 0).astype(np.int64)
    assert np.min(np.sum((B.T @ B) > 0, axis=1)[A.any(axis=0)]) > 256
    P, _, fa, fb = R.fit_parts(*csr, 700, 1, 0.6)
    SW = _restated(csr, 700, P, fa, fb)
    return csr, (P, fa, fb), {k: R.neighbours_from(*SW, k) for k in (7, 128)}


@pytest.mark.parametrize("band", [64, 320, 0])
@pytest.mark.parametrize("tied", [False, True])
def test_neighbors_more_candidates_than_the_pending_area(gpu_device, tied, band):
    csr, parts, want = _many_candidates(tied)
    for k in (7, 128):
        _check(gpu_device, csr, 700, k, band, parts, want=want[k])


def test_neighbors_sum_beyond_2_53_rounds_once(gpu_device):
    """A hand-made P table: 8 200 users rate items 0 and 1, every P is 2^40 but one 2^40 + 1, so S_01 = 8200 * 2^40 + 1 is odd
    and above 2^53: the conversion to double rounds, and the weight is the one the restatement forms from the rounded value."""
    U = 8200
    csr = _csr([[0, 1]] * U)
    P = np.full(2 * U, 2 ** 40, dtype=np.int64)
    P[2 * 4000 + 1] += 1                                               # P_{4000, 1}
    fa, fb = R.factors([U, U], 1, 0.6)
    S, W = _restated(csr, 2, P, fa, fb)
    assert int(S[0, 1]) == U * 2 ** 40 + 1 > 2 ** 53 and int(S[0, 1]) % 2 == 1 and int(float(S[0, 1])) != int(S[0, 1])
    assert int(S[1, 0]) == U * 2 ** 40
    want_id, want_w = _check(gpu_device, csr, 2, 1, 64, (P, fa, fb))
    assert want_id.tolist() == [[1, 0]] and np.all(want_w > 0)


def test_neighbors_sum_across_2_32(gpu_device):
    """Hand-made P: 0xFFFFFFFF and 1 add up to exactly 2^32, the carry out of the accumulator's low word; three times 2^31 and
    a lone 2^33 + 5 beside them."""
    csr = _csr([[0, 1, 2], [0, 1, 2], [0, 2, 3], [3]])
    P = np.array([7, 0xFFFFFFFF, 2 ** 31, 9, 1, 2 ** 31, 11, 2 ** 31, 2 ** 33 + 5, 3], dtype=np.int64)
    fa, fb = np.array([1.0, 0.5, 0.25, 1.0]), np.array([1.0, 1.0, 0.5, 0.125])
    S, _ = _restated(csr, 4, P, fa, fb)
    assert int(S[0, 1]) == 2 ** 32 and int(S[0, 2]) == 3 * 2 ** 31 and int(S[0, 3]) == 2 ** 33 + 5
    _check(gpu_device, csr, 4, 3, 64, (P, fa, fb))


@pytest.mark.parametrize("order", ["null", "identity", "reversed", "random"])
def test_neighbors_order(gpu_device, order):
    perm = {"null": None, "identity": np.arange(100), "reversed": np.arange(100)[::-1],
            "random": np.random.default_rng(1).permutation(100)}[order]
    csr, parts = _tie_block()
    _check(gpu_device, csr, 100, 25, 64, parts, order=perm)


def test_neighbors_two_runs_give_the_same_bits(gpu_device):
    csr, parts, _ = _many_candidates(False)
    runs = [_neighbors(gpu_device, csr, 700, 50, 128, *parts) for _ in range(2)]
    assert runs[0][0] == runs[1][0] == 0
    assert np.array_equal(runs[0][1].host(), runs[1][1].host()) and np.array_equal(_bits(runs[0][2].host()), _bits(runs[1][2].host()))


def test_neighbors_maximal_band(gpu_device):
    """The largest band (all of a CU's LDS) on a small problem: one band, most of it unused."""
    csr = _random_csr(30, 129, 0.2, True, 5)
    _check(gpu_device, csr, 129, 25, _lib.RK_RP3_MAX_BAND, _device_parts(gpu_device, csr, 129, 1, 0.6))


@pytest.mark.parametrize("k,band,drop,n_users", [(0, 64, None, None), (129, 64, None, None), (25, 96, None, None), (25, 32, None, None),
                                                 (25, _lib.RK_RP3_MAX_BAND + 64, None, None), (25, -64, None, None),
                                                 (25, 64, 0, None), (25, 64, 2, None), (25, 64, 6, None),
                                                 (25, 64, None, _lib.RK_RP3_MAX_USERS)])
def test_neighbors_refusals_write_nothing(gpu_device, k, band, drop, n_users):
    csr = _random_csr(40, 65, 0.2, False, 2)
    P, _, fa, fb = R.fit_parts(*csr, 65, 1, 0.6)
    rc, ids, w = _neighbors(gpu_device, csr, 65, k, band, P, fa, fb, drop=drop, n_users=n_users)
    assert rc == -22 and ids.untouched() and w.untouched() and "rk_rp3_neighbors" in _err()


# ------------------------------------------------------------------------------------- rk_rp3_scores / rk_rp3_pair_scores
@functools.lru_cache(maxsize=None)
def _score_csr(I):
    """40 users: user 0 with an empty row, user 1 with one item, users 2..4 with 63, 64 and 65 items and user 5 with 300 (as far
    as the catalogue goes), the rest random; ratings 1..5 and a few 127."""
    rng = np.random.default_rng(1000 + I)
    lens = np.minimum(np.r_[[0, 1, 63, 64, 65, 300], rng.integers(1, max(2, I // 3 + 1), size=34)], I)
    rows = [np.sort(rng.choice(I, size=int(n), replace=False)) for n in lens]
    vals = [np.where(rng.random(len(r)) < 0.1, 127, rng.integers(1, 6, size=len(r))) for r in rows]
    return _csr(rows, vals)


def _device_fit(dev, csr, I, k, alpha=1, beta=0.6):
    """The tables the device fits from its own parts (checked against the restatement by the tests above)."""
    parts = _device_parts(dev, csr, I, alpha, beta)
    rc, ids, w = _neighbors(dev, csr, I, k, 0, *parts)
    assert rc == 0, _err()
    return ids.host().reshape(k, I).copy(), w.host().reshape(k, I).copy()


def _scores(dev, csr, I, ids, w, users, band, drop=None, k=None, n_users=None):
    k = ids.shape[0] if k is None else k
    out = Out(len(users) * I, torch.float32, dev)
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int32))]
    args = [_lib.ptr(t) for t in d]
    if drop is not None:
        args[drop] = None
    rc = _call(_lib.lib().rk_rp3_scores, dev, len(csr[0]) - 1 if n_users is None else n_users, I, k, *args[:5], len(users), args[5],
               band, _lib.ptr(out.full))
    return rc, out


def _check_scores(dev, csr, I, ids, w, users, band):
    ok = [u if 0 <= u < len(csr[0]) - 1 else 0 for u in users]         # user 0 has no items: what an id out of range scores like
    want = R.scores(*csr, I, ids, w, ok)
    rc, out = _scores(dev, csr, I, ids, w, users, band)
    assert rc == 0, _err()
    got = out.host().reshape(len(users), I)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:10]
    return want


def _user_list():
    """Every user, then repeats, the empty user again and ids out of range."""
    return list(range(40)) + [5, 5, 0, 39, -1, 40, 2 ** 30]


@pytest.mark.parametrize("I,k,band", [(1, 5, 0), (2, 5, 0), (63, 128, 0), (64, 7, 0), (65, 128, 0), (200, 128, 0), (1000, 128, 0),
                                      (150, 50, 64), (200, 128, 64), (1000, 100, 512)])
def test_scores_catalogue_sizes_and_bands(gpu_device, I, k, band):
    """From the tables the device fitted.  k = 128 with lists longer than 64 takes both trips of the slot loop; I = 150 at a band
    of 64 is three column bands (64, 64, 22), I = 200 four, I = 1000 at 512 two; rows of 0, 1, 63, 64, 65 and 300 items."""
    csr = _score_csr(I)
    ids, w = _device_fit(gpu_device, csr, I, k)
    if k == 128 and I >= 200:
        assert np.sum(ids[64:] >= 0) > 0, "some lists are longer than 64"
    users = _user_list()
    want = _check_scores(gpu_device, csr, I, ids, w, users, band)
    assert np.all(_bits(want[0]) == 0) and np.all(_bits(want[-1]) == 0), "a user with no items scores +0.0 everywhere"
    if I > 2:
        assert want.max() > 0 and np.array_equal(_bits(want[5]), _bits(want[40]))


def test_scores_sum_in_ascending_item_order(gpu_device):
    """The hand-made table of tests/test_rp3beta_host.py: 1 + 2^-24 + 2^-24 taken in ascending order of the user's items is 1."""
    ids = np.full((1, 4), -1, dtype=np.int32)
    ids[0, 1:] = 0
    w = np.array([[0.0, 1.0, 2.0 ** -24, 2.0 ** -24]], dtype=np.float32)
    csr = _csr([[1, 2, 3]])
    want = _check_scores(gpu_device, csr, 4, ids, w, [0], 0)
    assert want[0, 0] == np.float32(1.0) and R.scores(*csr, 4, ids, w, [0], descending=True)[0, 0] != want[0, 0]
    rc, out = _pairs(gpu_device, csr, 4, ids, w, [0, 0], [0, 1])
    assert rc == 0 and out.host().tolist() == [1.0, 0.0]


def test_scores_all_padding_table(gpu_device):
    ids, w = np.full((7, 65), -1, dtype=np.int32), np.zeros((7, 65), dtype=np.float32)
    want = _check_scores(gpu_device, _score_csr(65), 65, ids, w, _user_list(), 0)
    assert np.all(_bits(want) == 0)


def test_scores_no_users(gpu_device):
    ids, w = np.full((3, 65), -1, dtype=np.int32), np.zeros((3, 65), dtype=np.float32)
    rc, out = _scores(gpu_device, _score_csr(65), 65, ids, w, [], 0)
    assert rc == 0 and out.untouched()


@pytest.mark.parametrize("k,band,drop,n_users", [(0, 0, None, None), (129, 0, None, None), (7, -64, None, None), (7, 96, None, None),
                                                 (7, 32, None, None), (7, _lib.RK_RP3_MAX_BAND + 64, None, None), (7, 0, 0, None),
                                                 (7, 0, 1, None), (7, 0, 5, None), (7, 0, None, 0)])
def test_scores_refusals_write_nothing(gpu_device, k, band, drop, n_users):
    ids, w = np.full((7, 65), -1, dtype=np.int32), np.zeros((7, 65), dtype=np.float32)
    rc, out = _scores(gpu_device, _score_csr(65), 65, ids, w, [1, 2, 3], band, drop=drop, k=k, n_users=n_users)
    assert rc == -22 and out.untouched() and "rk_rp3_scores" in _err()


def _pairs(dev, csr, I, ids, w, users, items, k=None, drop=None):
    n = len(users)
    out = Out(n, torch.float32, dev)
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int64),
                                np.asarray(items, dtype=np.int64))]
    args = [_lib.ptr(t) for t in d]
    if drop is not None:
        args[drop] = None
    rc = _call(_lib.lib().rk_rp3_pair_scores, dev, I, len(csr[0]) - 1, ids.shape[0] if k is None else k, *args, n, _lib.ptr(out.full))
    return rc, out


def test_pairs_equal_the_matrix_entries(gpu_device):
    """500 random pairs, seen items, empty rows, neighbourless items and ids out of range among them; k = 128 with long lists."""
    I, U = 150, 60
    csr = _random_csr(U, I, 0.3, True, 31, empty_rows=[0, 17], empty_cols=[4, 149])
    ids, w = _device_fit(gpu_device, csr, I, 128)
    assert np.all(ids[:, 4] == -1) and np.sum(ids[64:] >= 0) > 0
    rng = np.random.default_rng(32)
    users, items = rng.integers(0, U, size=500), rng.integers(0, I, size=500)
    ptr, idx, _ = csr
    users[:40] = np.repeat(np.arange(U), np.diff(ptr))[:40 * 7:7]      # seen items
    items[:40] = idx[:40 * 7:7]
    users[40:50], items[50:60], items[60:64] = 17, 4, 149
    bad = [(-1, 3), (U, 3), (3, -1), (3, I), (2 ** 40, 3), (3, 2 ** 40), (-2 ** 40, -2 ** 40), (U, I)]
    for n_, (u, i) in enumerate(bad):
        users[100 + n_], items[100 + n_] = u, i
    want = R.pair_scores(*csr, I, ids, w, users, items)
    rc, out = _pairs(gpu_device, csr, I, ids, w, users, items)
    assert rc == 0, _err()
    got = out.host()
    assert np.array_equal(_bits(got), _bits(want)), np.nonzero(_bits(got) != _bits(want))[0][:10]
    assert np.all(_bits(got[100:108]) == 0) and np.all(_bits(got[40:50]) == 0) and np.all(_bits(got[50:64]) == 0) and got[:40].any()
    rc, matrix = _scores(gpu_device, csr, I, ids, w, np.arange(U), 64)
    M = matrix.host().reshape(U, I)
    ok = np.ones(500, dtype=bool)
    ok[100:108] = False
    assert rc == 0 and np.array_equal(_bits(got[ok]), _bits(M[users[ok], items[ok]]))


def test_pairs_none(gpu_device):
    csr = _random_csr(10, 20, 0.3, False, 1)
    ids, w = np.full((3, 20), -1, dtype=np.int32), np.zeros((3, 20), dtype=np.float32)
    rc, out = _pairs(gpu_device, csr, 20, ids, w, [], [])
    assert rc == 0 and out.untouched()


@pytest.mark.parametrize("k,drop", [(0, None), (129, None), (7, 0), (7, 1), (7, 4), (7, 5), (7, 6)])
def test_pairs_refusals_write_nothing(gpu_device, k, drop):
    ids, w = np.full((7, 65), -1, dtype=np.int32), np.zeros((7, 65), dtype=np.float32)
    rc, out = _pairs(gpu_device, _score_csr(65), 65, ids, w, [1, 2], [3, 4], k=k, drop=drop)
    assert rc == -22 and out.untouched() and "rk_rp3_pair_scores" in _err()
