"""GPU tests of the ItemKNN kernels one entry point at a time (csrc/itemknn.hip) against the numpy restatement of the
definition (tests/_itemknn_restate.py).  Ids and the bit patterns of weights and scores are compared exactly: no tolerance, no
excluded case.  Every output buffer is pre-filled with NaN (ints: a sentinel) and carries a 64-element margin that must stay
as it was."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _itemknn_restate as R
from tests import _knn_restate as KR
from tests.test_knn_kernels_gpu import Out, _csr, _dev, _transpose

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _random_csr(U, I, density, explicit, seed, empty_rows=(), empty_cols=()):
    rng = np.random.default_rng(seed)
    A = rng.random((U, I)) < density
    A[list(empty_rows)] = False
    A[:, list(empty_cols)] = False
    rows = [np.nonzero(a)[0] for a in A]
    vals = [rng.integers(1, 6, size=len(r)) for r in rows] if explicit else None
    return _csr(rows, vals)


def _dense_csr(A):
    A = np.asarray(A)
    return _csr([np.nonzero(a)[0] for a in A], [a[np.nonzero(a)[0]] for a in A])


# ------------------------------------------------------------------------------------------------------ rk_itemknn_neighbors
def _neighbors(dev, csr, n_items, k, band, order=None, drop=None):
    ptr, idx, val = csr
    U = len(ptr) - 1
    colptr, crow, cval = _transpose(ptr, idx, val, n_items)
    rnorm = R.item_rnorm(R.dense(ptr, idx, val, n_items))
    ids, w = Out(max(k, 1) * n_items, torch.int32, dev), Out(max(k, 1) * n_items, torch.float32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, dev) for a in (ptr.astype(np.int32), idx, val, colptr, crow, cval, rnorm)]      # held until the call has returned
    d_order = None if order is None else _dev(np.asarray(order, dtype=np.int32), dev)
    args = [P(t) for t in d]
    if drop is not None:
        args[drop] = None
    rc = L.rk_itemknn_neighbors(U, n_items, *args, k, band, P(d_order), P(ids.full), P(w.full), S(dev))
    torch.cuda.synchronize()
    return rc, ids, w


def _check(dev, csr, n_items, k, band, want=None, **kw):
    want_id, want_w = R.neighbours(*csr, n_items, k) if want is None else want
    rc, ids, w = _neighbors(dev, csr, n_items, k, band, **kw)
    assert rc == 0, _lib.lib().rk_last_error()
    got_id, got_w = ids.host().reshape(k, n_items), w.host().reshape(k, n_items)
    assert np.array_equal(got_id, want_id), np.argwhere(got_id != want_id)[:10]
    assert np.array_equal(_bits(got_w), _bits(want_w)), np.argwhere(_bits(got_w) != _bits(want_w))[:10]
    return want_id, want_w


@pytest.mark.parametrize("U", [1, 5, 70])
@pytest.mark.parametrize("I", [1, 2, 3, 63, 64, 65, 129, 200])
def test_neighbors_shapes(gpu_device, I, U):
    """Every item is first, inside or last in some band of 64; k >= I - 1 pads, I = 1 has no candidate at all; user 0's row is
    empty when there are several users and item I - 2 has no rater."""
    csr = _random_csr(U, I, 0.5 if U < 70 else 0.15, (I + U) % 2 == 0, 100 * I + U, empty_rows=[0] if U > 1 else [],
                      empty_cols=[I - 2] if I > 2 else [])
    for k in (1, 2, 7, 64, 128):
        want_id, _ = _check(gpu_device, csr, I, k, 64)
        if k >= I:
            assert np.all(want_id[max(I - 1, 0):] == -1)
    if I > 2:
        assert np.all(want_id[:, I - 2] == -1) and not np.any(want_id == I - 2)


@pytest.mark.parametrize("band", [64, 128, 0])
@pytest.mark.parametrize("kind", ["implicit", "ratings", "value127"])
def test_neighbors_bands(gpu_device, kind, band):
    """I = 200: bands of 64 (last one 8 wide) and 128 (last one 72), and the automatic single band."""
    csr = list(_random_csr(90, 200, 0.12, kind != "implicit", 17, empty_rows=[3, 89], empty_cols=[0, 64, 199]))
    if kind == "value127":
        csr[2] = np.where(np.arange(len(csr[2])) % 3 == 0, np.float32(127), csr[2]).astype(np.float32)
    for k in (7, 50):
        _check(gpu_device, tuple(csr), 200, k, band)


@functools.lru_cache(maxsize=None)
def _tie_block():
    """70 users over 100 items: columns 10..49 are identical, the rest random."""
    rng = np.random.default_rng(5)
    A = (rng.random((70, 100)) < 0.2) * rng.integers(1, 6, size=(70, 100))
    A[:, 10:50] = A[:, [10]]
    assert A[:, 10].any()
    return _dense_csr(A)


@pytest.mark.parametrize("band", [64, 0])
@pytest.mark.parametrize("k", [7, 25, 39, 64])
def test_neighbors_block_of_identical_columns(gpu_device, k, band):
    """Each of the 40 identical columns has the 39 others tied at the top: with k below the block size the lowest ids win."""
    want_id, want_w = _check(gpu_device, _tie_block(), 100, k, band)
    top = min(k, 39)
    assert want_id[:top, 30].tolist() == [j for j in range(10, 50) if j != 30][:top] and len(np.unique(want_w[:top, 30])) == 1


@pytest.mark.parametrize("k", [1, 3, 5, 9, 10, 11])
def test_neighbors_tie_group_across_a_band_edge(gpu_device, k):
    """Columns 60..70 are identical and nothing else overlaps them: a cut inside the group keeps the lowest ids, whichever side
    of the edge between the bands [0, 64) and [64, 128) they lie on."""
    rng = np.random.default_rng(6)
    A = np.zeros((40, 130), dtype=np.int64)
    A[:20, :60] = rng.random((20, 60)) < 0.3
    A[:20, 71:] = rng.random((20, 59)) < 0.3
    A[20:, 60:71] = rng.integers(1, 6, size=(20, 1))
    want_id, _ = _check(gpu_device, _dense_csr(A), 130, k, 64)
    assert want_id[:, 60].tolist()[: min(k, 10)] == list(range(61, 71))[:k] and want_id[:, 70].tolist()[: min(k, 10)] == list(range(60, 70))[:k]


@pytest.mark.parametrize("band", [64, 128])
def test_neighbors_tie_group_in_a_later_band(gpu_device, band):
    """Columns 5..14 and 130..139 are all identical: item 5's list is full of ids 6..13 after the first band, and the ten equal
    candidates of a later band must not displace any of them."""
    rng = np.random.default_rng(7)
    A = ((rng.random((50, 200)) < 0.1) * rng.integers(1, 6, size=(50, 200))).astype(np.int64)
    col = rng.integers(1, 6, size=50) * (rng.random(50) < 0.5)
    A[:, 5:15] = col[:, None]
    A[:, 130:140] = col[:, None]
    want_id, want_w = _check(gpu_device, _dense_csr(A), 200, 8, band)
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
    assert np.min(np.sum((A.T @ A) > 0, axis=1)[A.any(axis=0)]) > 256
    return csr, {k: R.neighbours(*csr, 700, k) for k in (7, 128)}


@pytest.mark.parametrize("band", [64, 320, 0])
@pytest.mark.parametrize("tied", [False, True])
def test_neighbors_more_candidates_than_the_pending_area(gpu_device, tied, band):
    csr, want = _many_candidates(tied)
    for k in (7, 128):
        _check(gpu_device, csr, 700, k, band, want=want[k])


def test_neighbors_large_dot(gpu_device):
    """Two items co-rated by 1100 users at 127 but for one 2: the dot is odd and above 2^24, the conversion rounds
    (large_dot_odd of the DegSim restatement, transposed)."""
    p, i, v, n = KR.large_dot_odd()
    A = KR.dense(p, i, v, n).T                                         # 1100 users x 2 items
    csr = _dense_csr(A)
    D = A.T @ A
    assert D[0, 1] % 2 == 1 and D[0, 1] > 2 ** 24 and D[0, 0] < 2 ** 31
    want_id, want_w = _check(gpu_device, csr, 2, 1, 64)
    assert want_id.tolist() == [[1, 0]] and int(np.float32(D[0, 1])) != D[0, 1] and np.all(want_w > 0.99)


@pytest.mark.parametrize("order", ["null", "identity", "reversed", "random"])
def test_neighbors_order(gpu_device, order):
    perm = {"null": None, "identity": np.arange(100), "reversed": np.arange(100)[::-1],
            "random": np.random.default_rng(1).permutation(100)}[order]
    _check(gpu_device, _tie_block(), 100, 25, 64, order=perm)


def test_neighbors_maximal_band(gpu_device):
    """The largest band (all of a CU's LDS) on a small problem: one band, most of it unused."""
    _check(gpu_device, _random_csr(30, 129, 0.2, True, 5), 129, 25, _lib.RK_ITEMKNN_MAX_BAND)


@pytest.mark.parametrize("k,band,drop", [(0, 64, None), (129, 64, None), (25, 96, None), (25, 32, None),
                                         (25, _lib.RK_ITEMKNN_MAX_BAND + 64, None), (25, -64, None), (25, 64, 0), (25, 64, 6)])
def test_neighbors_refusals_write_nothing(gpu_device, k, band, drop):
    rc, ids, w = _neighbors(gpu_device, _random_csr(40, 65, 0.2, False, 2), 65, k, band, drop=drop)
    assert rc == -22 and ids.untouched() and w.untouched()
    assert "rk_itemknn_neighbors" in _lib.lib().rk_last_error().decode()


# --------------------------------------------------------------------------------------------------------- rk_itemknn_scores
def _tables(I, k, seed, padding=0.2):
    """Any table is a valid input: ids anywhere in [0, I) or -1 in any slot, positive weights."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, I, size=(k, I)).astype(np.int32)
    ids[rng.random((k, I)) < padding] = -1
    w = (rng.random((k, I)).astype(np.float32) + np.float32(2.0 ** -20)).astype(np.float32)
    w[ids < 0] = 0
    return ids, w


def _scores(dev, csr, I, ids, w, users, user_block, drop=None, k=None):
    k = ids.shape[0] if k is None else k
    out = Out(len(users) * I, torch.float32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int32))]
    args = [P(t) for t in d]
    if drop is not None:
        args[drop] = None
    rc = L.rk_itemknn_scores(I, k, *args[:5], len(users), args[5], user_block, P(out.full), S(dev))
    torch.cuda.synchronize()
    return rc, out


def _check_scores(dev, csr, I, ids, w, users, user_block):
    want = R.scores(*csr, I, ids, w, users)
    rc, out = _scores(dev, csr, I, ids, w, users, user_block)
    assert rc == 0, _lib.lib().rk_last_error()
    got = out.host().reshape(len(users), I)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:10]
    return want


@functools.lru_cache(maxsize=None)
def _score_csr(I):
    """40 users, user 0 with an empty row, ratings 1..5 and a few 127."""
    ptr, idx, val = _random_csr(40, I, 0.3, True, 1000 + I, empty_rows=[0])
    val = np.where(np.arange(len(val)) % 11 == 0, np.float32(127), val).astype(np.float32)
    return ptr, idx, val


def _user_list(nb, seed):
    """nb ids of the 40 users, user 0 (empty row) among them when nb > 1, repeats when nb > 2."""
    u = np.random.default_rng(seed).integers(0, 40, size=nb)
    if nb > 1:
        u[nb // 2] = 0
    if nb > 2:
        u[-1] = u[0]
    return u


@pytest.mark.parametrize("k", [1, 7, 128])
@pytest.mark.parametrize("I", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_scores_catalogue_sizes(gpu_device, I, k):
    """33 users under the automatic block of 16 (two full blocks and one user); I = 1000 splits the items over several workgroups."""
    users = _user_list(33, I + k)
    want = _check_scores(gpu_device, _score_csr(I), I, *_tables(I, k, I * 131 + k), users, 0)
    assert np.all(_bits(want[16]) == 0), "a user with an empty row scores +0.0 everywhere"


@pytest.mark.parametrize("user_block", [1, 2, 16, 0])
def test_scores_user_blocks(gpu_device, user_block):
    ub = user_block or 16
    ids, w = _tables(257, 7, 3)
    for nb in sorted({1, 2, max(ub - 1, 1), ub, ub + 1, 33}):
        _check_scores(gpu_device, _score_csr(257), 257, ids, w, _user_list(nb, nb), user_block)


@pytest.mark.parametrize("user_block", [3, 5, 8, 13])
def test_scores_other_user_blocks(gpu_device, user_block):
    """Blocks that are not the accumulator count of a kernel instance (4, 8, 16)."""
    ids, w = _tables(130, 5, 4)
    _check_scores(gpu_device, _score_csr(130), 130, ids, w, _user_list(33, user_block), user_block)


def test_scores_all_padding_table(gpu_device):
    ids, w = np.full((7, 65), -1, dtype=np.int32), np.zeros((7, 65), dtype=np.float32)
    want = _check_scores(gpu_device, _score_csr(65), 65, ids, w, _user_list(20, 1), 0)
    assert np.all(_bits(want) == 0)


def test_scores_restated_tables(gpu_device):
    """The tables the neighbour kernel produces (trailing padding, ties), every user once and in order."""
    csr = _score_csr(255)
    ids, w = R.neighbours(*csr, 255, 20)
    _check_scores(gpu_device, csr, 255, ids, w, np.arange(40), 0)


def test_scores_large_catalogue(gpu_device):
    """70 000 items: only two byte rows fit, so three users take two blocks, and the items are split over many workgroups."""
    I = 70000
    rng = np.random.default_rng(12)
    rows = [np.sort(rng.choice(I, size=n, replace=False)) for n in (900, 0, 1, 2500, 40)]
    rows[2] = np.array([I - 1])
    csr = _csr(rows, [rng.integers(1, 6, size=len(r)) for r in rows])
    ids, w = _tables(I, 2, 13)
    ids[0, :5000] = I - 1                                              # the last byte of a row is read
    w[0, :5000] = np.float32(0.5)
    want = _check_scores(gpu_device, csr, I, ids, w, [3, 2, 0], 0)
    assert want[1, 0] > 0
    rc, out = _scores(gpu_device, csr, I, ids, w, [3, 2, 0], 3)
    assert rc == -22 and out.untouched() and "user_block = 3" in _lib.lib().rk_last_error().decode()


@pytest.mark.parametrize("k,user_block,drop", [(0, 0, None), (129, 0, None), (7, -1, None), (7, 17, None), (7, 0, 0), (7, 0, 5)])
def test_scores_refusals_write_nothing(gpu_device, k, user_block, drop):
    ids, w = _tables(65, 7, 5)
    rc, out = _scores(gpu_device, _score_csr(65), 65, ids, w, [1, 2, 3], user_block, drop=drop, k=k)
    assert rc == -22 and out.untouched()
    assert "rk_itemknn_scores" in _lib.lib().rk_last_error().decode()


def test_scores_refuse_a_catalogue_beyond_the_limit(gpu_device):
    I = _lib.RK_ITEMKNN_MAX_ITEMS + 1
    ids, w = np.full((1, I), -1, dtype=np.int32), np.zeros((1, I), dtype=np.float32)
    csr = _csr([[0, I - 1], []])
    rc, out = _scores(gpu_device, csr, I, ids, w, [0, 1], 0)
    assert rc == -22 and out.untouched()
    msg = _lib.lib().rk_last_error().decode()
    assert str(I) in msg and str(_lib.RK_ITEMKNN_MAX_ITEMS) in msg


def test_scores_no_users(gpu_device):
    ids, w = _tables(65, 3, 6)
    rc, out = _scores(gpu_device, _score_csr(65), 65, ids, w, [], 0)
    assert rc == 0 and out.untouched()


# ---------------------------------------------------------------------------------------------------- rk_itemknn_pair_scores
def _pairs(dev, csr, I, ids, w, users, items):
    n = len(users)
    out = Out(n, torch.float32, dev)
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int64),
                                np.asarray(items, dtype=np.int64))]
    rc = L.rk_itemknn_pair_scores(I, len(csr[0]) - 1, ids.shape[0], *(P(t) for t in d), n, P(out.full), S(dev))
    torch.cuda.synchronize()
    return rc, out


def test_pairs_equal_the_matrix_entries(gpu_device):
    """500 random pairs, seen items, empty rows, neighbourless items and ids out of range among them."""
    I, U = 150, 60
    csr = _random_csr(U, I, 0.15, True, 31, empty_rows=[0, 17], empty_cols=[4, 149])
    ids, w = R.neighbours(*csr, I, 7)
    assert np.all(ids[:, 4] == -1)
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
    assert rc == 0, _lib.lib().rk_last_error()
    got = out.host()
    assert np.array_equal(_bits(got), _bits(want)), np.nonzero(_bits(got) != _bits(want))[0][:10]
    assert np.all(_bits(got[100:108]) == 0) and np.all(_bits(got[40:64]) == 0) and got[:40].any()
    rc, matrix = _scores(gpu_device, csr, I, ids, w, np.arange(U), 0)
    M = matrix.host().reshape(U, I)
    ok = np.ones(500, dtype=bool)
    ok[100:108] = False
    assert rc == 0 and np.array_equal(_bits(got[ok]), _bits(M[users[ok], items[ok]]))


def test_pairs_none(gpu_device):
    csr = _random_csr(10, 20, 0.3, False, 1)
    ids, w = _tables(20, 3, 2)
    rc, out = _pairs(gpu_device, csr, 20, ids, w, [], [])
    assert rc == 0 and out.untouched()
