"""GPU tests of the UserKNN kernels one entry point at a time (csrc/userknn.hip) and of the fit path (rk_itemknn_neighbors on
the transposed roles) against the numpy restatement of the definition (tests/_userknn_restate.py).  Every entry is fed from
device inputs of its own: the scoring entries from the restated tables or from hand-made ones, never from the device's own fit.
Ids and the bit patterns of weights and scores are compared exactly.  Every output buffer is pre-filled with NaN (ints: a
sentinel) and carries a 64-element margin that must stay as it was."""
import functools

import numpy as np
import pytest
import torch

from recad_amd import _lib
from tests import _knn_restate as K
from tests import _userknn_restate as R
from tests.test_itemknn_kernels_gpu import _bits, _random_csr
from tests.test_knn_kernels_gpu import Out, _csr, _dev, _transpose

pytestmark = pytest.mark.gpu
MAX_BAND = _lib.RK_USERKNN_MAX_BAND
BANDS = (64, 128, 0, MAX_BAND)


def _err():
    return _lib.lib().rk_last_error().decode()


def _scores(dev, csr, I, ids, w, users, normalize, band, drop=None, k=None, n_users=None, n_items=None):
    k = ids.shape[0] if k is None else k
    out = Out(len(users) * I, torch.float32, dev)
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int32))]   # held until the call has returned
    args = [_lib.ptr(t) for t in d]
    if drop is not None and drop < len(args):
        args[drop] = None
    rc = _lib.lib().rk_userknn_scores(len(csr[0]) - 1 if n_users is None else n_users, I if n_items is None else n_items, k, *args[:5],
                                      len(users), args[5], int(normalize), band, None if drop == 6 else _lib.ptr(out.full),
                                      _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out


def _check_scores(dev, csr, I, ids, w, users, normalize, band, want=None):
    if want is None:
        want = R.scores(*csr, I, ids, w, users, normalize)
    rc, out = _scores(dev, csr, I, ids, w, users, normalize, band)
    assert rc == 0, _err()
    got = out.host().reshape(len(users), I)
    assert np.array_equal(_bits(got), _bits(want)), (normalize, band, np.argwhere(_bits(got) != _bits(want))[:10])
    return want


def _pairs(dev, csr, I, ids, w, users, items, normalize, k=None, drop=None):
    n = len(users)
    out = Out(n, torch.float32, dev)
    d = [_dev(a, dev) for a in (ids, w, csr[0].astype(np.int32), csr[1], csr[2], np.asarray(users, dtype=np.int64),
                                np.asarray(items, dtype=np.int64))]
    args = [_lib.ptr(t) for t in d]
    if drop is not None and drop < len(args):
        args[drop] = None
    rc = _lib.lib().rk_userknn_pair_scores(I, len(csr[0]) - 1, ids.shape[0] if k is None else k, *args, n, int(normalize),
                                           None if drop == 7 else _lib.ptr(out.full), _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------ sizes and forms
@functools.lru_cache(maxsize=None)
def _sized(U, I):
    """(csr, the restated tables at k = 128, the users scored): ratings 1..5 with a few 127; the last user's row is empty when
    there are several, and one column has no rater.  The tables of a smaller k are the first k slots."""
    ptr, idx, val = _random_csr(U, I, 0.5 if I < 200 else 0.12, True, 7 * U + I, empty_rows=[U - 1] if U > 2 else [],
                                empty_cols=[I - 2] if I > 2 else [])
    val = np.where(np.arange(len(val)) % 11 == 3, np.float32(127), val).astype(np.float32)
    csr = (ptr, idx, val)
    ids, w = R.neighbours(*csr, I, 128)
    users = list(range(U)) if U <= 70 else list(range(0, U, 5)) + [U - 1, U - 2]
    return csr, ids, w, users + [0, 0, U - 1, -1, U, 2 ** 30]          # repeats and ids out of range


@pytest.mark.parametrize("I", [1, 63, 64, 65, 200, 1000])
@pytest.mark.parametrize("U", [1, 2, 5, 70, 300])
def test_scores_sizes_and_forms(gpu_device, U, I):
    """k = 1, 5, 64, 65 and 128 (one trip of the slot registers, exactly one, and two), both forms, the band going round 64, 128,
    automatic and the largest: at I = 1000 a row straddles 16 and 8 bands, at I = 200 four and two."""
    csr, ids128, w128, users = _sized(U, I)
    if U == 300:
        assert np.sum(ids128[64:] >= 0) > 0, "some lists are longer than 64"
    for n, k in enumerate((1, 5, 64, 65, 128)):
        ids, w = np.ascontiguousarray(ids128[:k]), np.ascontiguousarray(w128[:k])
        if k > U - 1:
            assert np.all(ids[max(U - 1, 0):] == -1)
        for normalize in (False, True):
            want = _check_scores(gpu_device, csr, I, ids, w, users, normalize, BANDS[(n + normalize) % 4])
            assert np.all(_bits(want[-3:]) == 0), "an id out of range scores +0.0 everywhere"
            assert np.array_equal(_bits(want[0]), _bits(want[-6])) and np.array_equal(_bits(want[0]), _bits(want[-5]))
    if U >= 5 and I >= 63:
        assert want.max() > 0


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("I", [200, 1000])
def test_scores_every_band_at_two_widths(gpu_device, I, band):
    csr, ids128, w128, users = _sized(70, I)
    ids, w = np.ascontiguousarray(ids128[:65]), np.ascontiguousarray(w128[:65])
    for normalize in (False, True):
        _check_scores(gpu_device, csr, I, ids, w, users, normalize, band)


# ------------------------------------------------------------------------------------------------------------ neighbour rows
@functools.lru_cache(maxsize=None)
def _row_lengths():
    """40 users over 1000 items with rows of 0, 1, 63, 64, 65, 127, 128, 129 (both sides of the length from which a row is
    searched for the band's segment) and 300 entries, the rest random; ratings 1..5 and a few 127."""
    rng = np.random.default_rng(77)
    lens = np.r_[[0, 1, 63, 64, 65, 127, 128, 129, 300], rng.integers(1, 200, size=31)]
    rows = [np.sort(rng.choice(1000, size=int(n), replace=False)) for n in lens]
    rows[1] = np.array([int(rows[8][5])])                              # the row of one overlaps the row of 300
    vals = [np.where(rng.random(len(r)) < 0.1, 127, rng.integers(1, 6, size=len(r))) for r in rows]
    csr = _csr(rows, vals)
    ids, w = R.neighbours(*csr, 1000, 39)
    return csr, ids, w


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("band", [64, 128, 512, 0])
def test_scores_neighbour_rows_of_every_length(gpu_device, band, normalize):
    """k = 39 = U - 1: everybody who overlaps is kept, so every row length is gathered by many users.  With a band narrower than
    the catalogue the rows of 129 and 300 entries are searched, the others strided whole and filtered; band 0 is one band."""
    csr, ids, w = _row_lengths()
    assert all(np.any(ids == v) for v in range(1, 9)) and not np.any(ids == 0)
    want = _check_scores(gpu_device, csr, 1000, ids, w, list(range(40)), normalize, band)
    assert np.all(_bits(want[0]) == 0) and want[1].max() > 0


# ------------------------------------------------------------------------------------------------------------ hand-made tables
def _hand_csr():
    """6 users over 130 items (three bands of 64); user 5 has no ratings."""
    rng = np.random.default_rng(3)
    A = (rng.random((6, 130)) < 0.4) * rng.integers(1, 6, size=(6, 130))
    A[5] = 0
    A[1, 64], A[2, 64], A[3, 64], A[1, 129] = 127, 1, 3, 4
    return _csr([np.nonzero(a)[0] for a in A], [a[np.nonzero(a)[0]] for a in A])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("band", [64, 0])
def test_scores_hand_made_tables(gpu_device, band, normalize):
    """Column u is user u's list: an id -1 in the middle, ids outside [0, U) (negative, U, 2^30), the same neighbour in two slots
    (added twice, in slot order), a neighbour with no ratings, weights of +0.0 (a denominator of exactly 0 at every column)."""
    csr = _hand_csr()
    ids = np.array([[1, 2, 3, 1, 1, -1],
                    [-1, 6, 1, 2, 2, -1],
                    [2, -7, 3, -1, 3, -1],
                    [2 ** 30, 3, -1, 5, 1, -1],
                    [3, 4, 4, 4, 2, -1]], dtype=np.int32)
    w = np.array([[0.9, 0.8, 0.7, 0.0, 0.75, 0.0],
                  [0.5, 0.7, 0.6, 0.0, 0.5, 0.0],
                  [0.4, 0.6, 0.5, 0.0, 0.25, 0.0],
                  [0.3, 0.3, 0.4, 0.0, 0.125, 0.0],
                  [0.2, 0.1, 0.3, 0.0, 0.0625, 0.0]], dtype=np.float32)
    want = _check_scores(gpu_device, csr, 130, ids, w, [0, 1, 2, 3, 4, 5, 2, 2], normalize, band)
    assert np.all(_bits(want[3]) == 0) and np.all(_bits(want[5]) == 0) and want[0].max() > 0 and want[2, 64] > 0
    users, items = np.repeat(np.arange(6), 130), np.tile(np.arange(130), 6)
    rc, out = _pairs(gpu_device, csr, 130, ids, w, users, items, normalize)
    assert rc == 0 and np.array_equal(_bits(out.host().reshape(6, 130)), _bits(want[:6]))


def test_scores_sum_in_ascending_slot_order(gpu_device):
    """The table of tests/test_userknn_host.py: 1 + 2^-24 + 2^-24 in ascending slot order is 1; the other way it carries."""
    csr = _csr([[], [0], [0], [0]])
    ids = np.array([[1], [2], [3]], dtype=np.int32).repeat(4, axis=1)
    w = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32).repeat(4, axis=1)
    want = _check_scores(gpu_device, csr, 4, ids, w, [0], False, 0)
    assert want[0, 0] == np.float32(1.0) and np.all(_bits(want[0, 1:]) == 0)
    up = _check_scores(gpu_device, csr, 4, np.ascontiguousarray(ids[::-1]), np.ascontiguousarray(w[::-1]), [0], False, 0)
    assert up[0, 0] == np.float32(1.0 + 2.0 ** -23)
    norm = _check_scores(gpu_device, csr, 4, ids, w, [0], True, 0)
    assert norm[0, 0] == np.float32(1.0) and np.all(_bits(norm[0, 1:]) == 0), "columns nobody rated: den = 0 gives +0.0"


def test_scores_value_127_and_ratings(gpu_device):
    csr = list(_random_csr(50, 150, 0.2, True, 12, empty_rows=[4]))
    for kind in ("ratings", "value127"):
        if kind == "value127":
            csr[2] = np.full(len(csr[2]), 127, dtype=np.float32)
        ids, w = R.neighbours(*csr, 150, 20)
        for normalize in (False, True):
            want = _check_scores(gpu_device, tuple(csr), 150, ids, w, list(range(50)), normalize, 64)
            assert want.max() > (126 if kind == "value127" and normalize else 1)


def test_scores_wide_catalogue(gpu_device):
    """70 000 items, two users, the automatic band: nine passes of 7 808 columns, rows of 3 000 entries searched per band."""
    rng = np.random.default_rng(70)
    I = 70000
    rows = [np.sort(rng.choice(I, size=3000, replace=False)) for _ in range(2)]
    rows[1][:50] = rows[0][:50]
    rows[0][-1] = rows[1][-1] = I - 1
    rows = [np.unique(r) for r in rows]
    csr = _csr(rows, [rng.integers(1, 6, size=len(r)) for r in rows])
    ids, w = R.neighbours(*csr, I, 3)
    assert ids[:, 0].tolist() == [1, -1, -1] and ids[:, 1].tolist() == [0, -1, -1]
    for normalize in (False, True):
        want = _check_scores(gpu_device, csr, I, ids, w, [0, 1, 1], normalize, 0)
        assert want[0, I - 1] > 0 and np.count_nonzero(want[0]) == len(rows[1])


def test_scores_no_users(gpu_device):
    csr, ids, w, _ = _sized(5, 65)
    rc, out = _scores(gpu_device, csr, 65, ids, w, [], False, 0)
    assert rc == 0 and out.untouched()


def test_scores_twice_give_the_same_bits(gpu_device):
    csr, ids, w, users = _sized(300, 1000)
    for normalize in (False, True):
        a, b = (_scores(gpu_device, csr, 1000, ids, w, users, normalize, 128) for _ in range(2))
        assert a[0] == b[0] == 0 and np.array_equal(_bits(a[1].host()), _bits(b[1].host()))


@pytest.mark.parametrize("k,normalize,band,drop,n_users,n_items", [
    (0, 0, 0, None, None, None), (129, 0, 0, None, None, None), (7, 2, 0, None, None, None), (7, -1, 0, None, None, None),
    (7, 1, -64, None, None, None), (7, 0, 96, None, None, None), (7, 0, 32, None, None, None), (7, 1, MAX_BAND + 64, None, None, None),
    (7, 0, 0, 0, None, None), (7, 0, 0, 1, None, None), (7, 0, 0, 2, None, None), (7, 0, 0, 3, None, None), (7, 0, 0, 4, None, None),
    (7, 0, 0, 5, None, None), (7, 0, 0, 6, None, None), (7, 0, 0, None, 0, None), (7, 0, 0, None, None, 0)])
def test_scores_refusals_write_nothing(gpu_device, k, normalize, band, drop, n_users, n_items):
    csr, ids128, w128, _ = _sized(5, 65)
    ids, w = np.ascontiguousarray(ids128[:7]), np.ascontiguousarray(w128[:7])
    rc, out = _scores(gpu_device, csr, 65, ids, w, [1, 2, 3], normalize, band, drop=drop, k=k, n_users=n_users, n_items=n_items)
    assert rc == -22 and out.untouched() and "rk_userknn_scores" in _err()


# ------------------------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("normalize", [False, True])
def test_pairs_equal_the_matrix_entries(gpu_device, normalize):
    """500 pairs, seen items, empty rows, raterless items and ids out of range among them; k = 128 with lists longer than 64."""
    U, I = 150, 90
    csr = _random_csr(U, I, 0.15, True, 31, empty_rows=[0, 17], empty_cols=[4, 89])
    ids, w = R.neighbours(*csr, I, 128)
    assert np.sum(ids[64:] >= 0) > 0 and np.all(ids[:, 17] == -1)
    rng = np.random.default_rng(32)
    users, items = rng.integers(0, U, size=500), rng.integers(0, I, size=500)
    ptr, idx, _ = csr
    users[:40] = np.repeat(np.arange(U), np.diff(ptr))[:40 * 7:7]      # seen items
    items[:40] = idx[:40 * 7:7]
    users[40:50], items[50:60], items[60:64] = 17, 4, 89
    bad = [(-1, 3), (U, 3), (3, -1), (3, I), (2 ** 40, 3), (3, 2 ** 40), (-2 ** 40, -2 ** 40), (U, I)]
    for n_, (u, i) in enumerate(bad):
        users[100 + n_], items[100 + n_] = u, i
    want = R.pair_scores(*csr, I, ids, w, users, items, normalize)
    rc, out = _pairs(gpu_device, csr, I, ids, w, users, items, normalize)
    assert rc == 0, _err()
    got = out.host()
    assert np.array_equal(_bits(got), _bits(want)), np.nonzero(_bits(got) != _bits(want))[0][:10]
    assert np.all(_bits(got[100:108]) == 0) and np.all(_bits(got[40:50]) == 0) and np.all(_bits(got[50:64]) == 0) and got[:40].any()
    rc, matrix = _scores(gpu_device, csr, I, ids, w, np.arange(U), normalize, 64)
    M = matrix.host().reshape(U, I)
    ok = np.ones(500, dtype=bool)
    ok[100:108] = False
    assert rc == 0 and np.array_equal(_bits(got[ok]), _bits(M[users[ok], items[ok]]))


def test_pairs_none(gpu_device):
    csr, ids, w, _ = _sized(5, 65)
    rc, out = _pairs(gpu_device, csr, 65, ids, w, [], [], False)
    assert rc == 0 and out.untouched()


@pytest.mark.parametrize("k,normalize,drop", [(0, 0, None), (129, 0, None), (7, 2, None), (7, -1, None), (7, 0, 0), (7, 0, 1),
                                              (7, 0, 2), (7, 0, 3), (7, 0, 4), (7, 1, 5), (7, 1, 6), (7, 1, 7)])
def test_pairs_refusals_write_nothing(gpu_device, k, normalize, drop):
    csr, ids128, w128, _ = _sized(5, 65)
    ids, w = np.ascontiguousarray(ids128[:7]), np.ascontiguousarray(w128[:7])
    rc, out = _pairs(gpu_device, csr, 65, ids, w, [1, 2], [3, 4], normalize, k=k, drop=drop)
    assert rc == -22 and out.untouched() and "rk_userknn_pair_scores" in _err()


# ------------------------------------------------------------------------------------------------------------ the fit path
def _fit(dev, csr, I, k, band):
    """rk_itemknn_neighbors on the transposed roles, as include/recad_hip.h writes the call."""
    ptr, idx, val = csr
    U = len(ptr) - 1
    colptr, crow, cval = _transpose(ptr, idx, val, I)
    rnorm_user = K.rnorm(R.dense(ptr, idx, val, I))
    ids, w = Out(k * U, torch.int32, dev), Out(k * U, torch.float32, dev)
    d = [_dev(a, dev) for a in (colptr, crow, cval, ptr.astype(np.int32), idx, val, rnorm_user)]     # held until the call has returned
    rc = _lib.lib().rk_itemknn_neighbors(I, U, *[_lib.ptr(t) for t in d], k, band, None, _lib.ptr(ids.full), _lib.ptr(w.full),
                                         _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return rc, ids, w


@pytest.mark.parametrize("U", [1, 5, 70])
@pytest.mark.parametrize("I", [1, 2, 63, 64, 65, 200])
def test_fit_on_the_transposed_roles(gpu_device, I, U):
    """The user-user tables, ids and bits, in candidate bands of 64 (two of them at U = 70) and the automatic one.  U = 1 has no
    candidate at all: every slot is padding, and the transposed call is sound there."""
    csr = _random_csr(U, I, 0.5 if I < 200 else 0.15, (I + U) % 2 == 0, 100 * I + U, empty_rows=[0] if U > 1 else [],
                      empty_cols=[I - 2] if I > 2 else [])
    for k, band in ((1, 64), (5, 0), (50, 64), (128, 0)):
        want_id, want_w = R.neighbours(*csr, I, k)
        rc, ids, w = _fit(gpu_device, csr, I, k, band)
        assert rc == 0, _err()
        got_id, got_w = ids.host().reshape(k, U), w.host().reshape(k, U)
        assert np.array_equal(got_id, want_id), np.argwhere(got_id != want_id)[:10]
        assert np.array_equal(_bits(got_w), _bits(want_w)), np.argwhere(_bits(got_w) != _bits(want_w))[:10]
        assert np.all(want_id[max(U - 1, 0):] == -1)
        if U > 1:
            assert np.all(want_id[:, 0] == -1) and not np.any(want_id == 0), "a user with no ratings is nobody's neighbour"
    if U == 70 and I >= 63:
        assert np.sum(want_id >= 0) > 70
